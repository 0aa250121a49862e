#!/usr/bin/env python3
"""Kernel times of the pair statistics (mhs_msim_pair_stats, csrc/pairstats.hip) next to the nearest-neighbour search
(mhe_msim_nearest, csrc/evaluate.hip) on the same rows, both in self mode, from the library's own launch timer (mh_profile_start /
mh_profile_stop: two HIP events around every launch).  Information only - profiles/pairstats_events.txt is one box's run of this.

    python tools/pairstats_events.py [--rows 512 4096 16384] [--calls 20] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from musediffusion_amd import _lib, metric  # noqa: E402


def unit_rows(n, seed):
    """non-negative rows whose three parts have unit norm, half of the entries exact zeros (the layout get_vectors writes)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = (0.05 + torch.rand(n, 56, device="cuda", generator=g)) * (torch.rand(n, 56, device="cuda", generator=g) >= 0.5)
    v[:, [0, 32, 44]] += 1.0
    for a, b in ((0, 32), (32, 44), (44, 56)):
        v[:, a:b] /= v[:, a:b].norm(dim=1, keepdim=True)
    return v.contiguous()


def timed(fn, calls):
    """kernel name -> (detail, [milliseconds]) of the library launches fn makes, over `calls` calls"""
    def run():
        for _ in range(calls):
            fn()
    out = {}
    for r in _lib.record_launches(run):
        out.setdefault(r.kernel, (r.detail, []))[1].append(r.ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096, 16384])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    lines = ["pair statistics next to the nearest-neighbour search, self mode, device %s" % name.value.decode(),
             "library launch timer, %d calls after 3 warm-up calls, microseconds per launch: median (min .. max)" % a.calls]
    for n in a.rows:
        v = unit_rows(n, n)
        runs = (("mhs_msim_pair_stats", lambda: metric.pair_stats(v, threshold=1 - 2.0 ** -16)),
                ("mhe_msim_nearest", lambda: metric.nearest(v, return_values=True)))
        lines.append("N = %d rows (%d ordered pairs)" % (n, n * (n - 1)))
        for label, fn in runs:
            for _ in range(3):
                fn()
            for kernel, (detail, ms) in timed(fn, a.calls).items():
                us = [1e3 * x for x in ms]
                lines.append("  %-20s %-34s %-32s %9.1f (%.1f .. %.1f)" % (label, kernel.split("(")[0][-34:], detail, statistics.median(us), min(us), max(us)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
