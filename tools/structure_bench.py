#!/usr/bin/env python3
"""Kernel time of the structure counts (mhm_structure_counts, csrc/structure.hip) next to mh_decode_events (csrc/decode.hip), the
kernel that writes its input, on the same 64 x 1024-token decoded batch and in the same run, from the library's own launch timer
(mh_profile_start / mh_profile_stop: two HIP events around every launch).  Information only - there is no threshold: it is one launch
beside a reverse loop.  profiles/structure_events.txt is one box's run of this.

    python tools/structure_bench.py [--rows 64 1] [--calls 50] [--out FILE]"""
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
from launch_times import timed  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402

BARS, NOTES_PER_BAR, L = 16, 12, 1024   # 192 notes and one chord per bar in a row of 1024 tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    lines = ["structure counts next to mh_decode_events on the same batch, device %s" % name.value.decode(),
             "rows of %d tokens from the tests' generator: %d bars of %d notes" % (L, BARS, NOTES_PER_BAR),
             "library launch timer, %d calls after 3 warm-up calls, microseconds per launch: median (min .. max)" % a.calls]
    g = np.random.default_rng(0)
    for B in a.rows:
        tokens, mask = (torch.from_numpy(x).cuda() for x in dr.make_dense_rows(g, B, L, BARS, NOTES_PER_BAR))
        dec = du.decode_tokens(tokens, mask)
        counts = dec.counts.cpu()
        assert not dec.status.any() and int(counts[:, 0].min()) == BARS * NOTES_PER_BAR
        sc = metric.structure_counts(dec, max_bars=512)
        assert int(sc.counts[:, 0].min()) == BARS * NOTES_PER_BAR and int(sc.counts[:, 2].max()) <= BARS + 1
        lines.append("B = %d  (notes [B, %d, 4])" % (B, dec.notes.shape[1]))
        forms = (("decode_tokens", lambda: du.decode_tokens(tokens, mask)),
                 ("counts, table of 64 bars", lambda: metric.structure_counts(dec, max_bars=64)),
                 ("counts, table of 512 bars", lambda: metric.structure_counts(dec, max_bars=512)),
                 ("counts and bars, 512 bars", lambda: metric.structure_counts(dec, max_bars=512, return_bars=True)))
        for label, fn in forms:
            for _ in range(3):
                fn()
            for kernel, us in timed(fn, a.calls).items():
                lines.append("  %-26s %-24s %8.1f (%.1f .. %.1f)" % (label, kernel, statistics.median(us), min(us), max(us)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
