"""Shared helpers of the split-precision census and parity matrix (imported by test modules; not a conftest).

* `FAMILY`: every `__global__` kernel of csrc/split.hip, read from the source.
* `census_key`: (kernel text, launch note, grid) -> census key.  The recorder's kernel text is the literal `split_gemm_kernel<T, MH_ACT_NONE>`:
  it never shows the part type, and a runtime argument selects most paths, so the key takes from the launch note the class of each
  argument that selects a path:
    all kernels            the part type (dtype=bf16x3 | f16x3);
    split_gemm_kernel      the output form, the bias form (0 / col / row), the residual, the non-temporal stores, whether the launch is
                           persistent (more tiles than blocks: the prefetch before the epilogue) and the K class - K = 32 (two stages, the
                           main loop and every in-loop issue skipped), K = 64 (the first in-loop issue sits in the peeled even stage), K > 64;
    split_gemm_ln_kernel   the same K class;
    split_attn_kernel      the instantiation (dh, waves) is in the text; the tail class (L % 64 == 0 or a masked last key tile);
    split_ln_kernel        ADD is in the text; the chunk class of H: H / 8 <= 64 (one round, lanes without a chunk), a multiple of 64 chunks
                           above that (every lane in every round) or ragged above that (the lane-dependent last round);
    pack and join          whether cols is a multiple of the 8 elements a thread moves.
* `record`: tests/gemm_census.py's recorder for this family -> [(key, note, grid)].
* `WORKLOADS`: the sampler's forward at the bench.py shapes `c2`, `c2-bertbase` (hidden size 768: no full-row tile, so the unfused
  out=2 GEMM followed by split_layernorm) and `c1`, each in both split modes, all eager."""
import os
import re

import gemm_census as gc

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musediffusion_amd", "csrc", "split.hip")
with open(_SRC) as _f:
    FAMILY = tuple(sorted(set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", _f.read()))))

DTYPES = ("bf16x3", "f16x3")
ACT_NAME = {0: "MH_ACT_NONE", 1: "MH_ACT_TANH", 2: "MH_ACT_GELU_ERF"}


def fields(note):
    return dict(t.split("=", 1) for t in note.split() if "=" in t)


def k_class(K):
    K = int(K)
    return "K=32" if K == 32 else ("K=64" if K == 64 else "K>64")


def gemm_key(dtype, act, out, bias, res, nt, persistent, K):
    """bias: "0" / "col" / "row" """
    return "split_gemm_kernel<T, %s> | %s out=%d bias=%s res=%d nt=%d persistent=%d %s" % (
        ACT_NAME[int(act)], dtype, int(out), bias, int(res), int(nt), int(persistent), k_class(K))


def gemm_ln_key(dtype, K):
    return "split_gemm_ln_kernel<T> | %s %s" % (dtype, k_class(K))


def attn_key(dtype, dh, L):
    waves = 8 if int(dh) == 64 and int(L) >= 256 else 4
    return "split_attn_kernel<T, %d%s> | %s tail=%d" % (int(dh), ", 8" if waves == 8 else "", dtype, int(int(L) % 64 != 0))


def h_class(H):
    nch = int(H) // 8
    return "chunks<=64" if nch <= 64 else ("chunks=64n" if nch % 64 == 0 else "chunks=ragged")


def ln_key(dtype, add, H):
    return "split_ln_kernel<T, %s> | %s %s" % ("true" if add else "false", dtype, h_class(H))


def mover_key(kernel, dtype, cols):
    """kernel: "pack" / "join" """
    return "split_%s_kernel<T> | %s cols%%8=%d" % (kernel, dtype, int(cols) % 8)


def census_key(kernel, note, grid=None):
    """(kernel text, launch note, blocks launched) -> census key, or None for a kernel outside csrc/split.hip"""
    name = " ".join(kernel.strip().strip("()").split())
    base = name.split("<")[0].strip()
    if base not in FAMILY:
        return None
    kv = fields(note)
    dt = kv.get("dtype", "?")
    if base == "split_gemm_kernel":
        if not all(f in kv for f in ("out", "bias", "res", "nt", "ntiles", "K")) or grid is None:
            return "%s | %s ?" % (name, dt)
        return "%s | %s out=%s bias=%s res=%s nt=%s persistent=%d %s" % (name, dt, kv["out"], kv["bias"], kv["res"], kv["nt"],
                                                                      int(int(kv["ntiles"]) > int(grid)), k_class(kv["K"].split("x")[-1]))
    if base == "split_gemm_ln_kernel":
        return "%s | %s %s" % (name, dt, k_class(kv["K"].split("x")[-1]) if "K" in kv else "?")
    if base == "split_attn_kernel":
        return "%s | %s tail=%s" % (name, dt, int(int(kv["L"]) % 64 != 0) if "L" in kv else "?")
    if base == "split_ln_kernel":
        return "%s | %s %s" % (name, dt, h_class(kv["H"]) if "H" in kv else "?")
    return "%s | %s cols%%8=%s" % (name, dt, int(kv["cols"]) % 8 if "cols" in kv else "?")


def _parse_with_grid(fn):
    """gemm_census.record_family hands the key function (kernel, note) only; the persistent class needs the grid of the same record"""
    recs = gc.record_family(fn, lambda kernel, note: (kernel, note) if census_key(kernel, note) is not None else None)
    return [(census_key(k[0], k[1], grid), note, grid) for k, note, grid in recs]


def record(fn):
    """fn() with the per-launch recorder on -> [(key, note, grid)] of its split.hip launches, in launch order"""
    return _parse_with_grid(fn)


def keys_of(fn):
    return [k for k, _, _ in record(fn)]


def _with(run):
    return lambda dev: run(dev, record)


WORKLOADS = {"fwd %s %s" % (w, dt): _with(gc._forward(w, dt)) for w in ("c2", "c2-bertbase", "c1") for dt in DTYPES}
