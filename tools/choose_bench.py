#!/usr/bin/env python3
"""Kernel times of choosing among candidates (csrc/choose.hip), from the library's own launch timer (mh_profile_start /
mh_profile_stop: two HIP events around every launch) and from HIP events around the Python calls:
  mhac_pair_fit at S songs x T tracks x K candidates of about `notes` notes a row, next to a torch restatement of the same counts
  on the same device and in the same run (all pairs of a song's notes as broadcast tensors, one song at a time), the two compared
  element for element before anything is timed;
  mhac_choose on random tables at (T, K) = (6, 4), (6, 8) and (20, 2), S songs each;
  what choosing adds to a batch: decode of the candidate batch, anchor_shift, pair_fit, fit_scores, choose_tracks and the gather
  of the chosen rows (sampling.choose_candidates + DecodedBatch.select), next to the decode of a batch of the chosen rows' size.
Information only - there is no threshold.  profiles/choose_events.txt is one box's run of this.

    python tools/choose_bench.py [--songs 8] [--tracks 6] [--candidates 4] [--notes 200] [--calls 50] [--out FILE]"""
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
from interplay_bench import BARS, META, event_timed  # noqa: E402
from launch_times import timed  # noqa: E402
from musediffusion_amd import _lib, metric, sampling  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402


def make_rows(g, B, tracks, K, notes, cap):
    """every row: about `notes` notes (+-10 %) over BARS bars of 4/4 on the sixteenth-note grid, each track in an octave of its own"""
    n = g.integers(notes - notes // 10, notes + notes // 10 + 1, size=B)
    start = g.integers(0, BARS * 16, size=(B, cap)) * 120
    arr = np.zeros((B, cap, 4), np.int32)
    arr[:, :, 0], arr[:, :, 1] = start, start + g.integers(1, 9, size=(B, cap)) * 120
    arr[:, :, 2] = 36 + 8 * (np.arange(B) // K % tracks)[:, None] + g.integers(0, 16, size=(B, cap))
    arr[:, :, 3] = 80
    counts3 = np.zeros((B, 3), np.int32)
    counts3[:, 0] = n
    return arr, counts3, np.tile(np.array(META, np.int32), (B, 1))


def torch_pair_fit(notes, counts3, S, T, K):
    """ticks and pairs of metric.pair_fit_raw for valid, unshifted rows, in torch operations, one song at a time"""
    B, cap = notes.shape[0], notes.shape[1]
    R = T * K
    live = (torch.arange(cap, device=notes.device).unsqueeze(0) < counts3[:, :1]).view(S, R * cap)
    per = notes.view(S, R * cap, 4)
    row = torch.arange(R * cap, device=notes.device) // cap
    other = (row.unsqueeze(0) // K != row.unsqueeze(1) // K)
    ticks, pairs = [], []
    for s in range(S):
        st, en, pi = per[s, :, 0], per[s, :, 1], per[s, :, 2]
        o = torch.minimum(en.unsqueeze(1), en.unsqueeze(0)) - torch.maximum(st.unsqueeze(1), st.unsqueeze(0))
        on = (o > 0) & other & live[s].unsqueeze(1) & live[s].unsqueeze(0)
        common = torch.where(on, o.clamp(max=65535), torch.zeros_like(o)).long()
        d = (pi.unsqueeze(1) - pi.unsqueeze(0)).abs() % 12
        ic = torch.minimum(d, 12 - d)
        shape = (R, cap, R, cap)
        pairs.append(torch.stack([(on & (ic == c)).view(shape).sum((1, 3)) for c in range(7)], 2))
        ticks.append(torch.stack([torch.where(ic == c, common, torch.zeros_like(common)).view(shape).sum((1, 3)) for c in range(7)], 2))
    return torch.cat(ticks).view(B, R, 7), torch.cat(pairs).view(B, R, 7)


def line(name, us, how):
    return "  %-52s %10.1f (%.1f .. %.1f)   %s" % (name, statistics.median(us), min(us), max(us), how)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--tracks", type=int, default=6)
    ap.add_argument("--candidates", type=int, default=4)
    ap.add_argument("--notes", type=int, default=200)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, T, K = a.songs, a.tracks, a.candidates
    B = S * T * K
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    g = np.random.default_rng(0)
    cap = a.notes + a.notes // 10
    notes, counts3, meta = (torch.from_numpy(x).cuda() for x in make_rows(g, B, T, K, a.notes, cap))
    fit = metric.pair_fit_raw(notes, counts3, meta, S, T, K)
    ticks, pairs = torch_pair_fit(notes, counts3, S, T, K)
    assert not fit.status.any() and torch.equal(fit.ticks, ticks) and torch.equal(fit.pairs, pairs), "the two restatements differ"
    lines = ["choosing among candidates, device %s" % name.value.decode(),
             "pair_fit: %d songs x %d tracks x %d candidates x about %d notes over %d bars: %d row pairs, %d note pairs that sound together" % (
                 S, T, K, a.notes, BARS, S * T * (T - 1) * K * K // 2, int(pairs.sum()) // 2),
             "%d calls after 3 warm-up calls, microseconds per call: median (min .. max)" % a.calls]
    kernel = lambda: metric.pair_fit_raw(notes, counts3, meta, S, T, K)  # noqa: E731
    restated = lambda: torch_pair_fit(notes, counts3, S, T, K)  # noqa: E731
    for _ in range(3):
        kernel()
        restated()
    for k, us in timed(kernel, a.calls).items():
        lines.append(line(k, us, "library launch timer"))
    lines.append(line("metric.pair_fit_raw", event_timed(kernel, a.calls), "HIP events around the call"))
    lines.append(line("torch restatement, one song at a time", event_timed(restated, max(3, a.calls // 5)), "HIP events around the call"))
    scores = lambda: metric.fit_scores(fit.ticks)  # noqa: E731
    scores()
    lines.append(line("metric.fit_scores (torch)", event_timed(scores, a.calls), "HIP events around the call"))
    lines.append("choose: random tables in +-10^6, every row eligible, %d songs" % S)
    for t, k in ((6, 4), (6, 8), (20, 2)):
        W = torch.randint(-10 ** 6, 10 ** 6, (S, t * k, t * k), device="cuda", dtype=torch.int64)
        call = lambda: metric.choose_tracks(W, S, t, k)  # noqa: E731
        for _ in range(3):
            call()
        for kn, us in timed(call, a.calls).items():
            lines.append(line("%s (T, K) = (%d, %d): %d combinations" % (kn, t, k, k ** t), us, "library launch timer"))
    # what choosing adds to a batch, on decodable rows: the candidate batch's decode against the chosen rows' decode, and the rest
    import decode_ref as dr                                              # tests/: the generator of decodable rows
    L = 320
    tokens, masks, _ = dr.make_batch(5, L, (dr.BATCH_KINDS * (B // len(dr.BATCH_KINDS) + 1))[:B])
    tokens, masks = torch.from_numpy(tokens).cuda(), torch.from_numpy(masks).cuda()
    dec = du.decode_tokens(tokens, masks)
    dec.meta[:, :3] = dec.meta[:1, :3]
    dec.meta[:, 5] = 644

    def added():
        res = sampling.choose_candidates(dec, S, T, K)
        return dec.select(res.rows)
    for _ in range(3):
        added()
    lines.append("per batch of %d candidate rows of %d tokens (%d decoded): what run_arrangement(candidates=%d) adds behind the sampler" % (
        B, L, int((dec.status == 0).sum()), K))
    lines.append(line("decode of %d rows instead of %d" % (B, S * T), [x - y for x, y in zip(
        event_timed(lambda: du.decode_tokens(tokens, masks), a.calls), event_timed(lambda: du.decode_tokens(tokens[:S * T], masks[:S * T]), a.calls))],
        "HIP events, difference of two calls"))
    lines.append(line("anchor_shift, pair_fit, fit_scores, choose, gather", event_timed(added, a.calls), "HIP events around the call"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
