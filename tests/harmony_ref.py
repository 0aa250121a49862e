"""Plain-Python restatement of the chord-fit rule (include/musehip_harmony.h), the model csrc/harmony.hip is compared with bit for bit.
Written from the rule's wording, one note at a time over Python lists and sets, NOT the way the kernel computes it: no bit masks, no
bisection, no reductions - the chord in force is found by walking the whole list under the rule for every note."""
import math

import numpy as np

OK, MASKED, BAD_META, BAD_COUNTS = range(4)

CHORD0, CHORD_NN = 195, 303
INTERVALS = ((0, 4, 7), (0, 4, 7, 10), (0, 4, 8), (0, 3, 6), (0, 3, 7), (0, 3, 7, 10), (0, 3, 6, 10), (0, 4, 7, 11), (0, 5, 7))
MAJOR, MINOR = (0, 2, 4, 5, 7, 9, 11), (0, 2, 3, 5, 7, 8, 10)
TICKS_PER_BAR = {627: 1920, 628: 1440, 629: 1440, 630: 2880}   # 480 ticks a beat times 4, 3, 3, 6 beats (4/4, 3/4, 6/8, 12/8)


def chord_tones(token):
    """the pitch classes of a chord token, or None when it names no chord"""
    token = int(token)
    if not 195 <= token <= 302:
        return None
    r, q = divmod(token - CHORD0, 9)
    return {(9 + r + i) % 12 for i in INTERVALS[q]}


def scale_tones(key_token):
    k = int(key_token) - 602
    assert 0 <= k < 24
    return {(k % 12 + i) % 12 for i in (MINOR if k >= 12 else MAJOR)}


def chord_in_force(chords, start):
    """index of the entry in force at `start`, or -1: the largest tick <= start, among equal ticks the last in list order"""
    at = -1
    for j, (tick, _) in enumerate(chords):
        if tick <= start and (at < 0 or tick >= chords[at][0]):
            at = j
    return at


def judge(note, chords, scale):
    """-> (pitch class, judged, chord tone, scale tone, length) of one note"""
    start, end, pitch = int(note[0]), int(note[1]), int(note[2])
    pc = pitch % 12                                         # Python's % is non-negative
    at = chord_in_force(chords, start)
    tones = chord_tones(chords[at][1]) if at >= 0 else None
    judged = tones is not None
    return pc, judged, judged and pc in tones, pc in scale, min(max(end - start, 0), 65535)


def row_counts(notes, chords, meta, valid=True, max_bars=0, max_notes=None, max_chords=None, n=None, c=None):
    """one row -> (counts [8], hist [12], bars [max_bars][4], status).  notes: rows of (start, end, pitch, velocity); chords: rows of
    (tick, token); n / c: the counts the row claims (default: the lists' lengths); a row that is not OK has zeros everywhere."""
    n = len(notes) if n is None else int(n)
    c = len(chords) if c is None else int(c)
    zero = ([0] * 8, [0] * 12, [[0] * 4 for _ in range(max_bars)])
    if not valid:
        return zero + (MASKED,)
    key, ts = int(meta[1]), int(meta[2])
    if not (602 <= key <= 625 and 627 <= ts <= 630):
        return zero + (BAD_META,)
    if not (0 <= n <= (len(notes) if max_notes is None else max_notes) and 0 <= c <= (len(chords) if max_chords is None else max_chords)):
        return zero + (BAD_COUNTS,)
    tpb = TICKS_PER_BAR[ts]
    scale = scale_tones(key)
    chords = [(int(t), int(k)) for t, k in chords[:c]]
    counts, hist, bars = [0] * 8, [0] * 12, [[0] * 4 for _ in range(max_bars)]
    for j in range(n):
        pc, judged, tone, in_scale, length = judge(notes[j], chords, scale)
        flags = (1, int(judged), int(tone), int(in_scale))
        for i in range(4):
            counts[i] += flags[i]
        counts[4] += length
        counts[5] += length if judged else 0
        counts[6] += length if tone else 0
        hist[pc] += 1
        start = int(notes[j][0])
        if start >= 0:
            k = start // tpb
            counts[7] = max(counts[7], k + 1)
            if k < max_bars:
                for i in range(4):
                    bars[k][i] += flags[i]
    return counts, hist, bars, OK


def batch_counts(notes, chords, counts3, meta, valid=None, max_bars=0):
    """[B, max_notes, 4], [B, max_chords, 2], [B, 3], [B, 11] arrays -> dict of int32 arrays as mhh_harmony_counts fills them"""
    B, max_notes, max_chords = len(notes), notes.shape[1], chords.shape[1]
    rows = []
    for b in range(B):
        n, c = int(counts3[b][0]), int(counts3[b][1])
        ok = 0 <= n <= max_notes and 0 <= c <= max_chords
        rows.append(row_counts(notes[b][:n].tolist() if ok else [], chords[b][:c].tolist() if ok else [], meta[b],
                               True if valid is None else bool(valid[b]), max_bars, max_notes, max_chords, n, c))
    return dict(counts=np.array([r[0] for r in rows], np.int32).reshape(B, 8), hist=np.array([r[1] for r in rows], np.int32).reshape(B, 12),
                bars=np.array([r[2] for r in rows], np.int32).reshape(B, max_bars, 4), status=np.array([r[3] for r in rows], np.int32))


def summary(counts, hist, region=None, rest=None):
    """the ratios of evaluation.HarmonyTotals.summary() from integer totals, in float64: counts [8] and hist [12] summed over the OK
    rows; region / rest: (judged, chord tones) inside and outside the bar range, or None"""
    div = lambda a, b: float(a) / float(b) if b else float("nan")  # noqa: E731
    notes, judged, tones, in_scale, ticks, jticks, tticks = (int(x) for x in counts[:7])
    total = sum(int(x) for x in hist)
    entropy = float("nan")
    if total:
        entropy = 0.0
        for x in hist:
            if x:
                p = float(x) / float(total)
                entropy -= p * math.log2(p)
    out = {"notes": notes, "judged": judged, "ch": div(judged - tones, judged), "ch_ticks": div(jticks - tticks, jticks),
           "out_of_scale": div(notes - in_scale, notes), "judged_share": div(judged, notes), "pitch_class_entropy": entropy}
    if region is not None:
        out.update(ch_region=div(region[0] - region[1], region[0]), ch_rest=div(rest[0] - rest[1], rest[0]),
                   judged_region=int(region[0]), judged_rest=int(rest[0]))
    return out
