"""bench.py on the GPU: a plain run times exactly --steps steps and reports nothing beside the headline, and --dump-outputs writes
the same arrays from two runs with the same arguments (small config 1 shape: the procedure, not the numbers)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import REPO  # noqa: E402


def run_bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    outs = []
    for sub in ("a", "b"):
        out = run_bench("--gpus", "1", "--workload", "c1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / sub))
        assert out["steps"] == 3 and out["config"]["repeats"]["regions"] == 1 and out["ms_per_step"] > 0
        assert abs(out["value"] * out["ms_per_step"] - 1e3) < 1.0
        for key in ("roofline", "kernels", "cpu_baseline", "secondary", "parity_mode"):
            assert key not in out, key
        outs.append({n: np.load(str(tmp_path / sub / (n + ".npy"))) for n in ("sample", "pred_xstart", "tokens")})
    a, b = outs
    assert a["sample"].shape == a["pred_xstart"].shape == (8, 128, 128) and a["sample"].dtype == np.float32
    assert a["tokens"].shape == (8, 128) and a["tokens"].dtype == np.float64
    assert np.isfinite(a["sample"]).all() and ((a["tokens"] >= 0) & (a["tokens"] < 729)).all()
    for n in a:
        assert np.array_equal(a[n], b[n]), n
