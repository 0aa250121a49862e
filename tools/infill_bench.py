#!/usr/bin/env python3
"""Kernel times of the infill plan and splice (mhi_infill_plan / mhi_infill_splice, csrc/infill.hip) next to mh_merge_and_mask
(csrc/encode.hip: the same kind of ragged row work, three launches) on the same rows, from the library's own launch timer
(mh_profile_start / mh_profile_stop: two HIP events around every launch).  Information only - there is no threshold: the two launches
are noise beside a reverse loop.  profiles/infill_events.txt is one box's run of this.

    python tools/infill_bench.py [--rows 64 1] [--len 2096] [--calls 50] [--out FILE]"""
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
from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd.utils import infill_util as iu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--len", type=int, default=2096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = a.len
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    lines = ["infill plan and splice next to mh_merge_and_mask on the same rows, device %s" % name.value.decode(),
             "rows of %d tokens from the tests' generator: 16 bars of 28 notes, bars 4..8 regenerated" % L,
             "library launch timer, %d calls after 3 warm-up calls, microseconds per launch: median (min .. max)" % a.calls]
    g = np.random.default_rng(0)
    for B in a.rows:
        rows = [dr.make_row(g, L, "clean", n_bars=16, notes_per_bar=28) for _ in range(B)]
        tokens = torch.from_numpy(np.stack([r[0] for r in rows])).cuda()
        mask = torch.from_numpy(np.stack([r[1] for r in rows])).cuda()
        sampled = torch.randint(0, 729, (B, L), dtype=torch.int32, device="cuda")
        # the note part of the same rows as mh_merge_and_mask's input: words [B, L] behind an 11-token meta
        m = (mask == 0).sum(1)
        words = torch.zeros(B, L, dtype=torch.int32, device="cuda")
        wlen = torch.zeros(B, dtype=torch.int32, device="cuda")
        for b in range(B):
            n = int((tokens[b] != 0).sum()) - int(m[b])
            words[b, :n] = tokens[b, int(m[b]):int(m[b]) + n]
            wlen[b] = n
        src = tokens[:, :11].contiguous()
        cap = B * (11 + 1 + 2 * L)
        ids, mk = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
        off = torch.empty(B + 1, dtype=torch.int64, device="cuda")
        mlen, mst = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")

        def merge():
            _lib.check(_lib.lib().mh_merge_and_mask(src.data_ptr(), None, words.data_ptr(), wlen.data_ptr(), None, ids.data_ptr(), mk.data_ptr(),
                                                    off.data_ptr(), mlen.data_ptr(), mst.data_ptr(), B, 11, L, cap, _lib.current_stream()))

        lines.append("B = %d" % B)
        for label, room, fields in (("whole notes, room 1", 1, "all"), ("whole notes, room 0", 0, "all"), ("pitch only", 0, "pitch")):
            plan = iu.plan_infill(tokens, mask, (4, 8), room, fields)
            assert not plan.status.any()
            fn = lambda: iu.splice_infill(iu.plan_infill(tokens, mask, (4, 8), room, fields), sampled)  # noqa: E731
            for _ in range(3):
                fn()
            for kernel, us in timed(fn, a.calls).items():
                lines.append("  %-22s %-24s %8.1f (%.1f .. %.1f)" % (label, kernel, statistics.median(us), min(us), max(us)))
        for _ in range(3):
            merge()
        for kernel, us in timed(merge, a.calls).items():
            lines.append("  %-22s %-24s %8.1f (%.1f .. %.1f)" % ("mh_merge_and_mask", kernel, statistics.median(us), min(us), max(us)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
