#!/usr/bin/env python3
"""Kernel time of the region rounding of an infill (csrc/region.hip): the mhr_constrain_regions launch beside mhg_constrain_rows on
the same class tables (alternating, so that both see the same clocks), from the library's own launch timer (mh_profile_start /
mh_profile_stop: two HIP events around every launch).  Rows of `--bars` bars whose interiors the plan selects, every one of them with
`--room` notes of room.  Information only - there is no threshold: one launch behind a reverse loop.  profiles/region_rounding.txt is
one box's run of this.

    python tools/region_bench.py [--B 64] [--L 1024] [--bars 8] [--calls 50] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import decode_ref as dr  # noqa: E402  (the tests' generator of ComMU-shaped rows)
from grammar_bench import timed  # noqa: E402
from musediffusion_amd import _lib, ops  # noqa: E402
from musediffusion_amd.utils import grammar_util as gu, infill_util as iu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--L", type=int, default=1024)
    ap.add_argument("--bars", type=int, default=8)
    ap.add_argument("--notes", type=int, default=6, help="notes per bar of the piece")
    ap.add_argument("--room", type=int, default=4, help="notes of room added to every selected bar")
    ap.add_argument("--E", type=int, default=128)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, L, E, V = a.B, a.L, a.E, 729
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    g = np.random.default_rng(0)
    rows = [dr.make_row(g, L, "clean", n_bars=a.bars, notes_per_bar=a.notes) for _ in range(B)]
    ids = torch.from_numpy(np.stack([r[0] for r in rows]).astype(np.int32)).cuda()
    mask = torch.from_numpy(np.stack([r[1] for r in rows]).astype(np.int32)).cuda()
    plan = iu.plan_infill(ids, mask, (0, a.bars), room=a.room)
    assert int((plan.status != 0).sum()) == 0
    W = (0.5 * torch.randn(V, E, generator=torch.Generator().manual_seed(1))).cuda()
    x = (0.5 * torch.randn(B * L, E, generator=torch.Generator().manual_seed(2))).cuda()
    bias = torch.zeros(V).cuda()
    bias[0] = 2.0
    cs, ci = ops.class_argmax(x, W, bias, 1)
    cs, ci = cs.view(B, L, 8), ci.view(B, L, 8)

    def both():
        gu.constrain_rows(cs, ci, plan.tokens, mask, (0, 63))
        return gu.constrain_regions(cs, ci, plan)

    for _ in range(3):
        tokens, res = both()
    s = res.summary()
    assert s["rows"]["ok"] == B, s
    lines = ["region rounding of an infill beside the row Viterbi on the same class tables, device %s" % name.value.decode(),
             "library launch timer, %d calls after 3 warm-up calls, microseconds per launch: median (min .. max)" % a.calls,
             "B = %d, L = %d (%d tokens), %d selected bars per row with room for %d notes each: %d masked slots in %d segments, "
             "%d notes and %d pads placed" % (B, L, B * L, a.bars, a.room, s["masked"], s["segments"], s["notes"], s["pads"])]
    for kernel, us in timed(both, a.calls).items():
        lines.append("  %-28s %9.1f (%.1f .. %.1f)" % (kernel, statistics.median(us), min(us), max(us)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
