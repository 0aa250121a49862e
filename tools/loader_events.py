#!/usr/bin/env python3
"""Time the stages of one training batch of the device-resident loader (musediffusion_amd/data/dataset.py) by device events, next to
the numpy restatement (tests/loader_ref.py, oracle/batch.py) on one CPU core.  Information only - nothing is asserted on the times.

    python tools/loader_events.py [--batch 64] [--rows 2048] [--reps 200] > profiles/loader_events.txt

The dataset is synthetic: rows of about 500 merged tokens in the ComMU layout.  Each stage is warmed, then timed as `reps` calls
between two events on the current stream; a stage includes the torch launches of its wrapper (random draws, allocations)."""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import loader_ref as lr  # noqa: E402
from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd import data as mdata  # noqa: E402
from musediffusion_amd.data import dataset as mds  # noqa: E402
from oracle import batch as ob  # noqa: E402


def make_rows(n, seed=3):
    g = random.Random(seed)
    rows = []
    for i in range(n):
        row = [g.randint(561, 600), (602, 623)[i % 2], 627, 633, 639, 644, 651, 660, 700, 720, 727]
        bars = g.randint(12, 20)
        for b in range(bars // 2):
            row += [432, g.randint(195, 302)]
        row.append(1)
        for _ in range(bars):
            row.append(2)
            for p in sorted(g.sample(range(432, 560), g.randint(5, 9))):
                row += [p, g.randint(131, 194), g.randint(9, 124), g.randint(304, 431)]
        row.append(1)
        rows.append(np.array(row, np.int32))
    return rows


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_events: no GPU - this tool measures on the device only")
    dev = "cuda"
    rows = make_rows(a.rows)
    values, offsets = lr.ragged(rows)
    mask = np.concatenate([(np.arange(len(r)) > np.nonzero(r == 1)[0][0]).astype(np.int32) for r in rows])
    lengths = np.array([len(r) for r in rows])
    ds = mds.MusicDataset({"input_ids": torch.from_numpy(values).to(dev), "input_mask": torch.from_numpy(mask).to(dev)},
                          torch.from_numpy(offsets).to(dev), lengths, 2096)
    corr = mdata.Corruptions(("mt", "mn", "rn", "rr"), 2, 0.5)
    loader = mds.MusicLoader(ds, a.batch, True, corruption=corr, use_bucketing=True, seq_len=2096, augment=mdata.Augment())
    torch.manual_seed(0)
    mdata.corruption.generator.seed(0)
    idx = torch.randperm(a.rows)[:a.batch]
    idx_d = idx.to(dev)
    total = int(lengths[idx.numpy()].sum())
    fields, off, _ = mdata.gather_rows(ds.fields, ds.offsets, idx_d, total)
    ids = fields["input_ids"]
    choices = corr.draw_choices(a.batch)
    width = int(lengths[idx.numpy()].max())
    stages = [
        ("gather (offsets + 2 fields)", lambda: mdata.gather_rows(ds.fields, ds.offsets, idx_d, total)),
        ("augment", lambda: mdata.augment_rows(ids, off)),
        ("per-sequence corruption (mt,mn,rn,rr; corr_max 2, corr_p 0.5)", lambda: corr(ids, off, per_sequence=True, choices=choices)),
        ("collate (3 fields)", lambda: mdata.collate_batches({"input_ids": ids, "correct_ids": ids, "input_mask": fields["input_mask"]}, off, width)),
        ("whole batch: MusicLoader.batch (host decisions included)", lambda: loader.batch(idx)),
    ]
    import ctypes
    name = ctypes.create_string_buffer(128)
    _lib.lib().mh_device_name(0, name, 128)
    print("loader stages, batch %d x %.0f tokens (%d tokens), dataset %d rows, device %s" % (a.batch, total / a.batch, total, a.rows, name.value.decode()))
    print("device: mean of %d calls between two events, ms per batch" % a.reps)
    for label, fn in stages:
        print("  %-64s %8.3f" % (label, timed(fn, a.reps)))
    # the numpy restatement of the same batch on one core (the reference itself spends O(tokens) interpreter steps per row on top)
    torch.set_num_threads(1)
    kc, bc = np.random.default_rng(0).integers(-6, 6, a.batch), np.random.default_rng(1).integers(-2, 3, a.batch)
    bvals, boff = ids.cpu().numpy(), off.cpu().numpy()
    g = np.random.default_rng(2)
    draws = dict(u=g.random((2, total)), new=np.stack([g.integers(131, 195, (2, total)), g.integers(3, 131, (2, total)), g.integers(304, 432, (2, total))], -1),
                 pairs=np.tile(np.array([[0, 1], [1, 2], [0, 2]], np.int32), (2, a.batch, 1, 1)))

    def host(fn, reps=5):
        fn()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) / reps * 1e3

    def host_gather():
        o, n, _ = lr.gather_offsets(offsets, idx.numpy(), total)
        for src in (values, mask):
            lr.gather_rows(src, offsets, idx.numpy(), o, n, np.zeros(total, np.int32))

    brows = lr.rows_of(bvals, boff)
    bmask = lr.rows_of(fields["input_mask"].cpu().numpy(), boff)
    print("numpy restatement, one CPU core, ms per batch")
    for label, fn in (("gather", host_gather), ("augment", lambda: lr.augment_rows(bvals, boff, kc, bc)),
                      ("per-sequence corruption", lambda: lr.corrupt_per_sequence(bvals, boff, choices, corr.corr_available, draws)),
                      ("collate", lambda: ob.collate(brows, bmask, brows, width))):
        print("  %-64s %8.3f" % (label, host(fn)))


if __name__ == "__main__":
    main()
