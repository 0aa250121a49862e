#!/usr/bin/env python3
"""Kernel time of the interplay counts (mha_interplay_counts, csrc/arrange.hip) at 64 songs x 6 tracks x 256 notes, from the
library's own launch timer (mh_profile_start / mh_profile_stop: two HIP events around every launch), next to a torch restatement of
the same counts on the same device and in the same run (all pairs of a song's notes as broadcast tensors, eight songs at a time;
HIP events around the call).  The two are compared element for element before anything is timed.  Information only - there is no
threshold: it is one launch beside a reverse loop.  profiles/interplay_events.txt is one box's run of this.

    python tools/interplay_bench.py [--songs 64] [--tracks 6] [--notes 256] [--calls 50] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from launch_times import timed  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402

META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]
BARS = 16


def event_timed(fn, calls):
    """[microseconds] per call of fn between two HIP events on the current stream"""
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return out


def make_songs(g, songs, tracks, notes):
    """every track: `notes` notes over BARS bars of 4/4 on the sixteenth-note grid, each track in an octave of its own"""
    B = songs * tracks
    start = g.integers(0, BARS * 16, size=(B, notes)) * 120
    arr = np.zeros((B, notes, 4), np.int32)
    arr[:, :, 0], arr[:, :, 1] = start, start + g.integers(1, 9, size=(B, notes)) * 120
    arr[:, :, 2] = 36 + 8 * (np.arange(B) % tracks)[:, None] + g.integers(0, 16, size=(B, notes))
    arr[:, :, 3] = 80
    counts3 = np.zeros((B, 3), np.int32)
    counts3[:, 0] = notes
    return arr, counts3, np.tile(np.array(META, np.int32), (B, 1)), (np.arange(B) // tracks).astype(np.int32)


def torch_counts(notes, songs, tracks, chunk=8):
    """the pairs and ticks of metric.interplay_counts for full, valid, unshifted rows laid out song-major, in torch operations"""
    n = notes.shape[1]
    per = notes.view(songs, tracks * n, 4)
    row = torch.arange(tracks * n, device=notes.device) // n
    other = (row.unsqueeze(0) != row.unsqueeze(1)).unsqueeze(0)
    pairs, ticks = [], []
    for s0 in range(0, songs, chunk):
        p = per[s0:s0 + chunk]
        st, en, pi = p[:, :, 0], p[:, :, 1], p[:, :, 2]
        o = torch.minimum(en.unsqueeze(2), en.unsqueeze(1)) - torch.maximum(st.unsqueeze(2), st.unsqueeze(1))
        on = (o > 0) & other
        common = torch.where(on, o.clamp(max=65535), torch.zeros_like(o)).long()
        dp = pi.unsqueeze(2) - pi.unsqueeze(1)
        d = dp.abs() % 12
        ic = torch.minimum(d, 12 - d)
        cols = [ic == c for c in range(7)] + [dp < 0, dp > 0]
        shape = (p.shape[0], tracks, n, tracks * n)
        pairs.append(torch.stack([(on & c).view(shape).sum((2, 3)) for c in cols], 2))
        ticks.append(torch.stack([torch.where(c, common, torch.zeros_like(common)).view(shape).sum((2, 3)) for c in cols], 2))
    return torch.cat(pairs).view(songs * tracks, 9), torch.cat(ticks).view(songs * tracks, 9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--tracks", type=int, default=6)
    ap.add_argument("--notes", type=int, default=256)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = ctypes.create_string_buffer(256)
    _lib.lib().mh_device_name(0, name, len(name))
    g = np.random.default_rng(0)
    notes, counts3, meta, song = (torch.from_numpy(x).cuda() for x in make_songs(g, a.songs, a.tracks, a.notes))
    ic = metric.interplay_counts_raw(notes, counts3, meta, None, song)
    pairs, ticks = torch_counts(notes, a.songs, a.tracks)
    assert not ic.status.any() and torch.equal(ic.pairs, pairs) and torch.equal(ic.ticks, ticks), "the two restatements differ"
    lines = ["interplay counts, device %s" % name.value.decode(),
             "%d songs x %d tracks x %d notes over %d bars: %d pairs that sound together, every one seen from both rows" % (
                 a.songs, a.tracks, a.notes, BARS, int(pairs[:, :7].sum()) // 2),
             "%d calls after 3 warm-up calls, microseconds per call: median (min .. max)" % a.calls]
    kernel = lambda: metric.interplay_counts_raw(notes, counts3, meta, None, song)  # noqa: E731
    for _ in range(3):
        kernel()
        torch_counts(notes, a.songs, a.tracks)
    for k, us in timed(kernel, a.calls).items():
        lines.append("  %-44s %10.1f (%.1f .. %.1f)   library launch timer" % (k, statistics.median(us), min(us), max(us)))
    us = event_timed(kernel, a.calls)
    lines.append("  %-44s %10.1f (%.1f .. %.1f)   HIP events around the call" % ("metric.interplay_counts_raw", statistics.median(us), min(us), max(us)))
    us = event_timed(lambda: torch_counts(notes, a.songs, a.tracks), a.calls)
    lines.append("  %-44s %10.1f (%.1f .. %.1f)   HIP events around the call" % ("torch restatement, 8 songs at a time", statistics.median(us), min(us), max(us)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
