"""bench.py's launcher logic (no GPU): `--gpus N` without a launcher starts N ranks through torch.distributed.run as a child
process; a WORLD_SIZE that disagrees with --gpus is an error, also when it is 1.  Also what a plain run leaves to --full, and the
files of --dump-outputs."""
import os
import subprocess
import sys

import pytest

from conftest import REPO


def test_world_size_mismatch_is_an_error_even_for_one_rank():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--gpus 2 but WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_self_launch_command(monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, "call", fake_call)
    with pytest.raises(SystemExit) as e:
        bench.self_launch(4, ["--gpus", "4", "--steps", "3"])
    assert e.value.code == 7                                           # the parent exits with the child's code
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-5:] == [os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_main_self_launches_when_no_launcher(monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "1"])
    called = {}

    def fake_launch(n, argv):
        called["n"], called["argv"] = n, argv
        raise SystemExit(0)
    monkeypatch.setattr(bench, "self_launch", fake_launch)
    with pytest.raises(SystemExit):
        bench.main()
    assert called == {"n": 2, "argv": ["--gpus", "2", "--steps", "1"]}


def test_plain_run_times_the_headline_only():
    """A plain `--gpus 1 --steps N --warmup W` run times exactly N steps and measures nothing beside them; --full brings back the
    roofline / kernel tables, the CPU baseline, the secondary block and the repeated regions, each of which can still be switched off."""
    sys.path.insert(0, REPO)
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.repeats, a.full, a.dump_outputs) == (7, 2, 0, False, None)
    assert a.no_cpu_baseline and a.no_kernel_timing and a.no_secondary
    f = bench.parse_args(["--steps", "7", "--full"])
    assert f.repeats == 4 and not (f.no_cpu_baseline or f.no_kernel_timing or f.no_secondary)
    f = bench.parse_args(["--full", "--no-secondary", "--repeats", "2"])
    assert f.repeats == 2 and f.no_secondary and not f.no_cpu_baseline


def test_dump_outputs_types_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: float32 for floating tensors (float64 kept), float64 for integers; above the byte budget a fixed sample of each."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    x = torch.randn(4, 8, dtype=torch.bfloat16)
    tok = torch.arange(32, dtype=torch.int64).reshape(4, 8)
    bench.dump_outputs(str(tmp_path / "a"), {"x": x, "d": torch.ones(3, dtype=torch.float64), "tokens": tok})
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("x", "d", "tokens")}
    assert got["x"].dtype == np.float32 and np.array_equal(got["x"], x.float().numpy())
    assert got["d"].dtype == np.float64 and got["tokens"].dtype == np.float64 and np.array_equal(got["tokens"], tok.numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 1000)
    big = torch.randn(1000)
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big})
    b, c = np.load(str(tmp_path / "b" / "big.npy")), np.load(str(tmp_path / "c" / "big.npy"))
    assert b.nbytes <= 1000 and b.size == 250 and np.array_equal(b, c) and np.isin(b, big.numpy()).all()
