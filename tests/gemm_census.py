"""Shared helpers of the GEMM census and parity tests (imported by test modules; not a conftest).

* `philox7` / `dense_keep`: the dense dropout sites' keep flags restated on the host (numpy) - Philox4x32-7 keyed by the seed at counter
  ((row N + col) / 8, offset), 16 bits per element (csrc/common.h: drop_keep8).
* `record` (`record_family` for another kernel family: tests/attention_census.py): runs a callable with the library's per-launch recorder on (_lib.record_launches) and returns the GEMM-family
  launches as census keys: the kernel's template text as launched (it carries EPI, ACT, the epilogue form and the DMA bits) plus the
  `tile=` field of the launch note (which config `C` stood for).  Never call it inside a hipGraph capture.
* `WORKLOADS`: the eager runs the census records, at the shapes bench.py uses (dispatch depends on M); `run(dev, rec)` records with `rec`
  (default: `record`)."""
import numpy as np

GEMM_FAMILY = ("gemm_kernel", "gemm_big_kernel", "gemm_strip_kernel", "gemm_tn_kernel", "split_gemm_kernel", "split_gemm_ln_kernel")


def philox7(c, k0, k1, rounds=7):
    """Philox4x32 with `rounds` rounds (7: the dropout sites; 10: the truncated normal, tests/step_ref.py) on uint64 arrays holding 32-bit
    words: counter words c[0..3], key (k0, k1) -> 4 output words"""
    c = [np.asarray(x).astype(np.uint64) for x in c]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    M0, M1, W0, W1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & MASK, p1 & MASK, n2 & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def dense_keep(rows, cols, p, seed, offset):
    """keep flags [rows, cols] (bool) of a dense dropout site: element e = row cols + col draws 16 bits of Philox output e / 8"""
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    g = np.arange(rows * cols // 8, dtype=np.uint64)
    c = philox7([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full(g.shape, offset & 0xFFFFFFFF, np.uint64),
                 np.full(g.shape, offset >> 32, np.uint64)], seed & 0xFFFFFFFF, seed >> 32)
    keep = np.zeros((g.size, 8), dtype=bool)
    for w in range(4):
        keep[:, 2 * w] = (c[w] & np.uint64(0xFFFF)) >= np.uint64(thr)
        keep[:, 2 * w + 1] = (c[w] >> np.uint64(16)) >= np.uint64(thr)
    return keep.reshape(rows, cols)


def census_key(kernel, note):
    """(kernel text, launch note) -> census key, or None for a kernel outside the GEMM family"""
    name = kernel.strip().strip("()").strip()
    if name.split("<")[0].strip() not in GEMM_FAMILY:
        return None
    kv = dict(t.split("=", 1) for t in note.split() if "=" in t)
    key = "%s | tile=%s" % (" ".join(name.split()), kv.get("tile", "?"))
    # where the template text names a parameter instead of its value, the note carries it: the 128 x 128 kernel's epilogue kind and
    # operand type, the split GEMM's output form
    if name.startswith("gemm_kernel"):
        key += " epi=%s dtype=%s" % (kv.get("epi", "?"), kv.get("dtype", "?"))
    if name.startswith("split_gemm_kernel"):
        key += " out=%s" % kv.get("out", "?")
    return key


def record(fn):
    """fn() with the per-launch recorder on -> [(key, note)] of its GEMM-family launches, in launch order"""
    return [(k, note) for k, note, _ in record_family(fn, census_key)]


def record_family(fn, key_of):
    """fn() with the per-launch recorder on -> [(key, note, grid)] of the launches `key_of(kernel text, note)` gives a key (not None), in
    launch order; grid = blocks in x, as launched"""
    from musediffusion_amd import _lib
    keyed = ((key_of(r.kernel, r.detail), r) for r in _lib.record_launches(fn))
    return [(k, r.detail, r.grid) for k, r in keyed if k is not None]


# ------------------------------------------------------------------------------------------------------------- census workloads
def _bench():
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench
    return bench


def _forward(workload, dtype):
    def run(dev, rec=record):
        import torch
        bench = _bench()
        c = bench.WORKLOADS[workload]
        model, _ = bench.build(c, dtype, dev, seed=0)
        g = torch.Generator().manual_seed(11)
        x = torch.randn(c["B"], c["L"], c["E"], generator=g).to(dev)
        t = torch.randint(0, c["T"], (c["B"],), generator=g).to(dev)
        with torch.no_grad():
            return rec(lambda: model(x, t))
    return run


def _reverse_step(workload):
    """one eager p_sample step with the nearest-embedding rounding: the captured step's launches, run one by one"""
    def run(dev, rec=record):
        import torch
        bench = _bench()
        c = bench.WORKLOADS[workload]
        model, diff = bench.build(c, "bf16", dev, seed=0)
        diff.rng_mode, diff.rng_seed, diff.rng_stream, diff.use_graph = "philox", 105, 0, False
        loop = bench.make_loop(model, diff, c, "p", dev, 0, 2)
        with torch.no_grad():
            loop.begin()
            keys = rec(lambda: loop.advance(0))
            loop.finish()
        return keys
    return run


def _train(workload, p, B=None, L=None):
    """one training micro-step (training_losses forward + backward) in train mode with dropout p"""
    def run(dev, rec=record):
        import torch
        from musediffusion_amd import synthetic
        bench = _bench()
        c = dict(bench.WORKLOADS[workload])
        c["B"], c["L"] = B or c["B"], L or c["L"]
        model, diff = bench.build(c, "bf16", dev, seed=0)
        model.dropout.p = p
        model.bert_hidden_dropout = model.bert_attention_dropout = p
        model.train().requires_grad_(True)
        batch = {k: v.to(dev) for k, v in synthetic.training_batch(c["B"], c["L"], seed=1).items()}
        t = torch.randint(0, c["T"], (c["B"],), generator=torch.Generator().manual_seed(7)).to(dev)

        def step():
            model.zero_grad(set_to_none=True)
            diff.training_losses(model, t, model_kwargs=batch)["loss"].mean().backward()
        step()          # (lazy weight preparation and workspaces outside the recorded step)
        return rec(step)
    return run


# name -> run(device) -> [(key, note)]
WORKLOADS = {
    "fwd c2 bf16": _forward("c2", "bf16"),
    "fwd c2 fp32": _forward("c2", "fp32"),
    "fwd c2 bf16x3": _forward("c2", "bf16x3"),
    "fwd c2 f16x3": _forward("c2", "f16x3"),
    "fwd c2-bertbase bf16": _forward("c2-bertbase", "bf16"),
    "reverse step c2": _reverse_step("c2"),
    "train 32x1024 dropout 0.1": _train("train", 0.1),
    "train 32x1024 dropout 0": _train("train", 0.0),
    "train 8x128 (op-per-node tape)": _train("c1", 0.1),
}
