"""Shared helpers of the sampling-step census and parity matrix (imported by test modules; not a conftest).

* `FAMILY`: every `__global__` kernel of csrc/elementwise.hip, csrc/norm.hip, csrc/rounding.hip and csrc/headtail.hip, read from the
  sources, plus the two rounding helpers at the end of csrc/gemm.hip (row_sqnorm_f32_kernel, argbest_reduce_kernel).
* `census_key`: (kernel text, launch note) -> census key.  The recorder's kernel text carries the template arguments as launched
  (`step_epilogue4_kernel<false, true, true>`, `vocab_argmax_kernel<1>`, `ln_panel4_kernel<16, ADD>`); where a runtime argument selects a
  path the text does not show, the launch note does and the key takes its class: the update kernels' x0 source, mask form, per-batch
  coefficients, noise source and whether the slot fold runs; the LayerNorms' input and output type and whether position and time rows
  are added; the fused tail's update, its kind, noise source and mask form.
* `record`: tests/gemm_census.py's recorder for this family -> [(key, note, grid)].
* `WORKLOADS`: the GEMM census' three forwards, one p and one ddim step of config 2 with the default fusion settings, the same p step
  with fuse_rounding, fuse_noise and round_in_forward switched off in turn, and one generation plus one modification on the seq_len 128
  shape from token ids to final tokens (gather, q_sample, the logits argmax).  All eager."""
import os
import re

import gemm_census as gc

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musediffusion_amd", "csrc")
_GLOBAL = re.compile(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(")


def _kernels(name):
    with open(os.path.join(_CSRC, name)) as f:
        return set(_GLOBAL.findall(f.read()))


GEMM_HELPERS = ("row_sqnorm_f32_kernel", "argbest_reduce_kernel")
assert set(GEMM_HELPERS) <= _kernels("gemm.hip")
FAMILY = tuple(sorted(set().union(*(_kernels(n) for n in ("elementwise.hip", "norm.hip", "rounding.hip", "headtail.hip"))) | set(GEMM_HELPERS)))
EXEMPT = ("spin_kernel",)                # idles a wave for a time: no result to compare
EPILOGUES = ("step_epilogue_kernel", "step_epilogue4_kernel")
LAYERNORMS = ("ln_kernel", "ln_panel_kernel", "ln_panel4_kernel")


def fields(note):
    return dict(t.split("=", 1) for t in note.split() if "=" in t)


def epilogue_key(name, x0, mask, cpb, noise, fold=None):
    """name: the kernel text (`step_epilogue4_kernel<true, true>`); fold: only the SLOTS forms have one"""
    k = "%s | x0=%s mask=%s cpb=%d noise=%s" % (name, x0, mask, int(cpb), noise)
    return k if fold is None else k + " fold=%d" % int(fold)


def ln_key(name, x, out=None, add=0):
    k = "%s | x=%s" % (name, x)
    return (k + " out=%s" % out if out else k) + " add=%d" % int(add)


def tail_key(name, upd, ddim=0, noise="none", mask="none"):
    return "%s | upd=0" % name if not upd else "%s | upd=1 ddim=%d noise=%s mask=%s" % (name, int(ddim), noise, mask)


def census_key(kernel, note):
    """(kernel text, launch note) -> census key, or None for a kernel outside the family"""
    name = " ".join(kernel.strip().strip("()").split())
    base = name.split("<")[0].strip()
    if base not in FAMILY:
        return None
    kv = fields(note)
    g = lambda k: kv.get(k, "?")
    if base in EPILOGUES:
        slots = name.count(",") >= 1          # <DDIM, SLOTS[, RNG]>
        return "%s | x0=%s mask=%s cpb=%s noise=%s" % (name, g("x0"), g("mask"), g("cpb"), g("noise")) + (" fold=%s" % g("fold") if slots else "")
    if base == "ln_kernel":
        return "%s | x=%s out=%s add=%s" % (name, g("x"), g("out"), g("add"))
    if base in LAYERNORMS:
        return "%s | x=%s add=%s" % (name, g("x"), g("add"))
    if base == "tail_fused_kernel" and "upd" in kv:
        return "%s | upd=0" % name if kv["upd"] == "0" else "%s | upd=1 ddim=%s noise=%s mask=%s" % (name, g("ddim"), g("noise"), g("mask"))
    return name


def record(fn):
    """fn() with the per-launch recorder on -> [(key, note, grid)] of its launches of this family, in launch order"""
    return gc.record_family(fn, census_key)


def keys_of(fn):
    return [k for k, _, _ in record(fn)]


def _with(run):
    return lambda dev: run(dev, record)


def _step(kind, **off):
    """one eager reverse step of config 2 (tests/gemm_census.py: _reverse_step) of the given kind, with fusion switches turned off"""
    def run(dev):
        import torch
        bench = gc._bench()
        c = bench.WORKLOADS["c2"]
        model, diff = bench.build(c, "bf16", dev, seed=0)
        diff.rng_mode, diff.rng_seed, diff.rng_stream, diff.use_graph = "philox", 105, 0, False
        for k, v in off.items():
            setattr(diff, k, v)
        loop = bench.make_loop(model, diff, c, kind, dev, 0, 2)
        with torch.no_grad():
            loop.begin()
            recs = record(lambda: loop.advance(0))
            loop.finish()
        return recs
    return run


def _sample(mode):
    """sampling.generate / sampling.modify on the seq_len 128 shape, 3 reverse iterations, eager: ids -> embeddings -> loop -> tokens"""
    def run(dev):
        import torch
        from musediffusion_amd import sampling, synthetic
        bench = gc._bench()
        c = bench.WORKLOADS["c1"]
        model, diff = bench.build(c, "bf16", dev, seed=0)
        diff.use_graph = False
        cond = synthetic.generation_batch(c["B"], c["L"], seed=1)
        torch.manual_seed(3)
        if mode == "generate":
            return record(lambda: sampling.generate(model, diff, cond, t_enc=3, sharded=False))
        return record(lambda: sampling.modify(model, diff, cond, step=4, strength=0.75, sharded=False))
    return run


FORWARDS = ("fwd c2 bf16", "fwd c2 fp32", "fwd c2-bertbase bf16")
# name -> run(device) -> [(key, note, grid)]
WORKLOADS = {name: _with(gc.WORKLOADS[name]) for name in FORWARDS}
WORKLOADS["p step c2"] = _step("p")
WORKLOADS["ddim step c2"] = _step("ddim")
WORKLOADS["p step c2, fuse_rounding off"] = _step("p", fuse_rounding=False)
WORKLOADS["p step c2, fuse_noise off"] = _step("p", fuse_noise=False)
WORKLOADS["p step c2, round_in_forward off"] = _step("p", round_in_forward=False)
WORKLOADS["generate 8x128"] = _sample("generate")
WORKLOADS["modify 8x128"] = _sample("modify")
