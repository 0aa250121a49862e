#!/usr/bin/env python3
"""Time the 1NNC of a set of N rows by device events: metric.ONNC_sets (get_vectors, one fused nearest-neighbour
launch: csrc/evaluate.hip) next to metric.ONNC (one get_vectors, three exact-fp32 GEMMs with their pad casts, two multiplies,
fill_diagonal_, argmax over the materialised N x N matrix), and the nearest-neighbour stage of each alone.  Information only -
nothing is asserted on the times.

    python tools/evaluate_events.py [--sizes 100,4096] [--reps 200] > profiles/evaluate_events.txt

The rows are synthetic note sequences in the ComMU layout (4 bars of 4 - 6 notes: tests/decode_ref.py's generator), the first half
standing for the ground truth and the second for the generated set.  Each figure is the mean of `reps` back-to-back calls of the
Python wrapper between two events on the current stream, after five warm-up calls; the wrapper's torch work is inside it."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import decode_ref as dr  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402


def make_rows(n, L=112, seed=5):
    g = np.random.default_rng(seed)
    rows, lengths = np.zeros((n, L), np.int32), np.zeros(n, np.int32)
    for b in range(n):
        notes = dr.make_notes(g, 4, int(g.integers(4, 7)))
        rows[b, :len(notes)], lengths[b] = notes, len(notes)
    return rows, lengths


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def gemm_nearest(vec):
    sim = metric._similarity(vec, vec)
    sim.fill_diagonal_(0)
    return torch.argmax(sim, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,4096")
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_events: no GPU - this tool measures on the device only")
    name = ctypes.create_string_buffer(128)
    _lib.lib().mh_device_name(0, name, 128)
    print("1NNC of N rows (N / 2 ground truth, N / 2 generated), device %s" % name.value.decode())
    print("mean of %d calls between two events, ms per call" % a.reps)
    for n in (int(s) for s in a.sizes.split(",")):
        rows, lengths = make_rows(n)
        tok, ln = torch.from_numpy(rows).cuda(), torch.from_numpy(lengths).cuda()
        h = n // 2
        vec = metric.get_vectors(tok, ln)
        same = torch.equal(metric.nearest(vec).long(), gemm_nearest(vec))
        print("N = %d (the two paths pick the same neighbours: %s)" % (n, same))
        for label, fn in (("metric.ONNC_sets   (get_vectors over both halves, fused nearest, count)", lambda: metric.ONNC_sets(tok[:h], tok[h:], ln[:h], ln[h:])),
                          ("metric.ONNC        (get_vectors, 3 GEMMs + casts, product, argmax)", lambda: metric.ONNC(tok, ln)),
                          ("  nearest stage alone: metric.nearest (one launch)", lambda: metric.nearest(vec)),
                          ("  nearest stage alone: GEMM path (_similarity, fill_diagonal_, argmax)", lambda: gemm_nearest(vec))):
            print("  %-74s %8.3f" % (label, timed(fn, a.reps)))


if __name__ == "__main__":
    main()
