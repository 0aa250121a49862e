#!/usr/bin/env python3
"""Kernel time of the grammar-constrained rounding (csrc/grammar.hip) at bench.py's final-argmax shape: mhg_class_argmax beside
mh_logits_argmax on the same inputs (alternating, so that both see the same clocks), and the mhg_constrain_rows launch alone, from
the library's own launch timer (mh_profile_start / mh_profile_stop: two HIP events around every launch).  Information only - there is
no threshold: two launches behind a reverse loop.  profiles/grammar_decode.txt is one box's run of this.

    python tools/grammar_bench.py [--config c2] [--calls 50] [--out FILE]"""
import argparse
import ctypes
import functools
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import decode_ref as dr  # noqa: E402  (the tests' generator of ComMU-shaped metas)
import launch_times  # noqa: E402
from musediffusion_amd import _lib, ops  # noqa: E402
from musediffusion_amd.utils import grammar_util as gu  # noqa: E402

SHAPES = {"c2": dict(B=64, L=512, E=128, V=729), "c1": dict(B=8, L=128, E=128, V=729), "ref-default": dict(B=16, L=2096, E=500, V=729)}
BARS = 8
# the kernels here are template instantiations: named by their whole text, without the launch macro's parentheses (tools/region_bench.py too)
timed = functools.partial(launch_times.timed, name=lambda kernel: kernel.strip("()"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["c2"], choices=sorted(SHAPES))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    lines = ["grammar-constrained rounding at the final-argmax shape of bench.py's configs, device %s" % name.value.decode(),
             "library launch timer, %d calls after 3 warm-up calls, microseconds per launch: median (min .. max)" % a.calls]
    g = np.random.default_rng(0)
    for cfg in a.config:
        s = SHAPES[cfg]
        B, L, E, V = s["B"], s["L"], s["E"], s["V"]
        meta, chord = dr.make_meta(g, BARS, 1)
        ids = np.zeros((B, L), np.int32)
        ids[:, :len(meta) + len(chord)] = meta + chord
        mask = np.ones((B, L), np.int32)
        mask[:, :len(meta) + len(chord) + 1] = 0
        ids_d, mask_d = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
        W = (0.5 * torch.randn(V, E, generator=torch.Generator().manual_seed(1))).cuda()
        x = (0.5 * torch.randn(B * L, E, generator=torch.Generator().manual_seed(2))).cuda()
        bias = torch.zeros(V).cuda()
        bias[0] = 2.0
        wn = ops.row_sqnorm(W)
        lines.append("%s: B = %d, L = %d, E = %d, V = %d (%d tokens), %d bars in every meta" % (cfg, B, L, E, V, B * L, BARS))
        for mode, aux, plain in ((1, bias, lambda: ops.logits_argmax(x, W, bias)), (2, wn, lambda: ops.distance_argmax(x, W, wn))):
            def both():
                plain()
                ops.class_argmax(x, W, aux, mode)
            for _ in range(3):
                both()
            t = timed(both, a.calls)
            med = {k: statistics.median(v) for k, v in t.items()}
            for kernel, us in t.items():
                lines.append("  mode %d  %-28s %9.1f (%.1f .. %.1f)" % (mode, kernel, med[kernel], min(us), max(us)))
            lines.append("  mode %d  class_argmax / vocab_argmax = %.3f" % (mode, med["class_argmax_kernel<%d>" % mode] / med["vocab_argmax_kernel<%d>" % mode]))
        cs, ci = ops.class_argmax(x, W, bias, 1)
        cs, ci = cs.view(B, L, 8), ci.view(B, L, 8)
        for bars in ("exact", "decodable", (0, 63)):
            fn = lambda: gu.constrain_rows(cs, ci, ids_d, mask_d, bars)  # noqa: E731
            for _ in range(3):
                tokens, res = fn()
            assert int((res.status != 0).sum()) == 0
            for kernel, us in timed(fn, a.calls).items():
                lines.append("  bars %-10s %-28s %9.1f (%.1f .. %.1f)" % (bars if isinstance(bars, str) else "%d..%d" % bars, kernel,
                                                                         statistics.median(us), min(us), max(us)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
