#!/usr/bin/env python3
"""Throughput of the device batch producers / token validators at a BASELINE-sized batch
(512 sequences, ~1000 tokens each), with the numpy oracle (= the reference's per-token Python loops restated) beside it; then
the decode path (csrc/decode.hip) on 512 x 1024 generated rows beside its numpy restatement (profiles/decode_events.txt); then the
encode path (csrc/encode.hip) on 512 rows of about 500 notes (profiles/encode_events.txt)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from musediffusion_amd import data as mdata  # noqa: E402
from musediffusion_amd.utils import decode_util as mdec  # noqa: E402
from oracle import batch as ob  # noqa: E402

rng = np.random.default_rng(0)
rows = []
for _ in range(512):
    seq = list(rng.integers(560, 729, 11)) + [0]
    for k in range(int(rng.integers(200, 252))):
        if k % 24 == 0:
            seq.append(2)
        seq += [int(rng.integers(432, 560)), int(rng.integers(131, 195)), int(rng.integers(3, 131)), int(rng.integers(304, 432))]
    seq.append(1)
    rows.append(np.array(seq, np.int32))
v, off = mdata.to_ragged(rows, "cuda")
n = v.numel()
u = torch.rand(n, device="cuda")
new = torch.stack([torch.randint(131, 195, (n,)), torch.randint(3, 131, (n,)), torch.randint(304, 432, (n,))], 1).int().cuda()
pairs = mdata.corruption._draw_bar_pairs(v, off, 3)
col = mdata.collate_batches({"input_ids": v}, off, 1024)
notes, lens = col["input_ids"][:, 12:].contiguous(), (col["length"] - 12)


def timeit(fn, reps=50):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


cases = [
    ("masking_token", lambda: mdata.masking_token(v, off, 0.3, u=u), n * 12, lambda i: ob.masking_token(rows[i], np.zeros(len(rows[i])), 0.3)),
    ("masking_note", lambda: mdata.masking_note(v, off, 0.5, u=u), n * 12, lambda i: ob.masking_note(rows[i], np.zeros(len(rows[i])), 0.5)),
    ("randomize_note", lambda: mdata.randomize_note(v, off, 0.5, u=u, new_tokens=new), n * 24,
     lambda i: ob.randomize_note(rows[i], np.zeros(len(rows[i])), np.zeros((len(rows[i]), 3), np.int32), 0.5)),
    ("random_rotating", lambda: mdata.random_rotating(v, off, 3, pairs=pairs), n * 8, lambda i: ob.random_rotating(rows[i], [(0, 1)] * 3)),
    ("collate (1 field)", lambda: mdata.collate_batches({"input_ids": v}, off, 1024), n * 4 + 512 * 1024 * 4, None),
    ("validate_tokens", lambda: mdec.validate_tokens(notes, lens), n * 4, lambda i: ob.validate(rows[i][12:], len(rows[i]) - 12)),
]
print("%d sequences, %d tokens" % (len(rows), n))
for name, fn, nbytes, cpu in cases:
    us = timeit(fn)
    line = "%-18s %8.1f us  %7.1f GB/s algorithmic" % (name, us, nbytes / us / 1e3)
    if cpu is not None:
        t0 = time.perf_counter()
        for i in range(0, 64):
            cpu(i)
        dt = (time.perf_counter() - t0) / 64 * len(rows)
        line += "   | numpy/python oracle, 1 core: %8.1f ms per batch (%.0fx)" % (dt * 1e3, dt * 1e6 / us)
    print(line, flush=True)

# ---- decode: sampled token rows -> restored note sequences -> notes / chord markers (csrc/decode.hip), 512 x 1024 from the tests' row
# generator (rows that decode and rows of every failure kind), event-timed per kernel, beside the numpy restatement of the same path
# (tests/decode_ref.py = the reference's per-sequence host loop restated) on one core.  A single box's numbers; nothing gates on them.
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import decode_ref as dr  # noqa: E402
from musediffusion_amd._lib import current_stream, lib  # noqa: E402

tok_np, mask_np, kinds = dr.make_batch(0, 1024, [dr.BATCH_KINDS[i % len(dr.BATCH_KINDS)] for i in range(512)])
tok, msk = torch.from_numpy(tok_np).cuda(), torch.from_numpy(mask_np).cuda()
B, L, LD, MAXN, MAXC = 512, 1024, 2048, 513, 1025
restored, rlen, meta = torch.empty(B, LD, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, 11, dtype=torch.int32, device="cuda")
st0, st = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
notes_d, chords_d = torch.zeros(B, MAXN, 4, dtype=torch.int32, device="cuda"), torch.zeros(B, MAXC, 2, dtype=torch.int32, device="cuda")
counts = torch.empty(B, 3, dtype=torch.int32, device="cuda")


def restore():
    lib().mh_restore_chord(tok.data_ptr(), msk.data_ptr(), restored.data_ptr(), rlen.data_ptr(), meta.data_ptr(), st0.data_ptr(), B, L, LD, current_stream())


def events():
    st.copy_(st0)                                        # the status is in / out: start every repetition from restore_chord's
    lib().mh_decode_events(restored.data_ptr(), rlen.data_ptr(), meta.data_ptr(), None, 0, notes_d.data_ptr(), chords_d.data_ptr(),
                           counts.data_ptr(), st.data_ptr(), B, LD, MAXN, MAXC, current_stream())


us_restore = timeit(restore)
us_copy = timeit(lambda: st.copy_(st0))
us_events = timeit(events) - us_copy
us_all = timeit(lambda: mdec.decode_tokens(tok, msk))
t0 = time.perf_counter()
ref_rows = dr.decode_rows(tok_np[:64], mask_np[:64], LD, MAXN, MAXC)
host_ms = (time.perf_counter() - t0) / 64 * B * 1e3
torch.cuda.synchronize()
assert [int(s) for s in st[:64].cpu()] == [r["status"] for r in ref_rows]
n_ok = int((st == 0).sum())
print("decode: %d rows x %d tokens (%d decode, %d notes, %d chord markers)" % (B, L, n_ok, int(counts[:, 0].sum()), int(counts[:, 1].sum())))
print("%-18s %8.1f us" % ("mh_restore_chord", us_restore))
print("%-18s %8.1f us" % ("mh_decode_events", us_events))
print("%-18s %8.1f us  (allocation, zero fill and both kernels)   | numpy/python restatement, 1 core: %8.1f ms per batch (%.0fx the two kernels)"
      % ("decode_tokens", us_all, host_ms, host_ms * 1e3 / (us_restore + us_events)), flush=True)

# ---- encode: notes + chord progression -> event words -> merged model rows (csrc/encode.hip), 512 rows of about 500 notes over 16
# measures from the tests' generator (encode_ref.bench_items: every time signature, 480 / 96 / 220 / 384 ticks per beat), event-timed per
# entry point, beside the numpy restatement on one core.  tools/make_golden_encode.py --time-reference times the reference itself on
# the same rows where the reference is installed.  A single box's numbers; nothing gates on them.
import encode_ref as er  # noqa: E402
from musediffusion_amd.utils import encode_util as menc  # noqa: E402

items = er.bench_items()
p = er.pack(items)
B, LD, S = len(items), 4096, 11
d = {k: torch.from_numpy(a).cuda() for k, a in p.items()}
words, wlen = torch.empty(B, LD, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
ecounts, est = torch.empty(B, 2, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
src = torch.randint(560, 729, (B, S), dtype=torch.int32, device="cuda")
cap = B * (S + 1 + 2 * LD)
ids, mask = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
moff, mlen, mst = torch.empty(B + 1, dtype=torch.int64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")


def encode():
    lib().mh_encode_events(d["notes"].data_ptr(), d["n_notes"].data_ptr(), d["params"].data_ptr(), d["slots"].data_ptr(), d["n_slots"].data_ptr(),
                           words.data_ptr(), wlen.data_ptr(), ecounts.data_ptr(), est.data_ptr(), B, p["notes"].shape[1], p["slots"].shape[1], LD,
                           current_stream())


def merge():
    lib().mh_merge_and_mask(src.data_ptr(), None, words.data_ptr(), wlen.data_ptr(), est.data_ptr(), ids.data_ptr(), mask.data_ptr(),
                            moff.data_ptr(), mlen.data_ptr(), mst.data_ptr(), B, S, LD, cap, current_stream())


us_encode, us_merge = timeit(encode), timeit(merge)
us_py = timeit(lambda: menc.merge_and_mask(src, *(lambda e: (e.words, e.lengths, e.status))(menc.encode_notes(*(d[k] for k in ("notes", "n_notes", "params", "slots", "n_slots"))))))
t0 = time.perf_counter()
ref = er.encode_rows({k: a[:32] for k, a in p.items()}, LD)
for w, _, _ in ref:
    er.merge_row(np.zeros(S, np.int32), w)
host_ms = (time.perf_counter() - t0) / 32 * B * 1e3
torch.cuda.synchronize()
assert [int(x) for x in est[:32].cpu()] == [r[2] for r in ref] and all(words[b, :len(r[0])].cpu().tolist() == r[0] for b, r in enumerate(ref))
print("encode: %d rows, %d notes (%d rows encode, %d words, %d merged tokens)" % (B, int(p["n_notes"].sum()), int((est == 0).sum()), int(wlen.sum()), int(moff[-1])))
print("%-18s %8.1f us" % ("mh_encode_events", us_encode))
print("%-18s %8.1f us  (three launches)" % ("mh_merge_and_mask", us_merge))
print("%-18s %8.1f us  (allocations and both entry points)   | numpy/python restatement, 1 core: %8.1f ms per batch (%.0fx the two entry points)"
      % ("encode + merge (py)", us_py, host_ms, host_ms * 1e3 / (us_encode + us_merge)), flush=True)
