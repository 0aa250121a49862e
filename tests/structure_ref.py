"""Plain-Python restatement of the structure rule (include/musehip_structure.h), the model csrc/structure.hip is compared with bit for
bit.  Written from the rule's wording, one note at a time over Python lists, sets and ints, NOT the way the kernel computes it: no
atomics, no reductions, no tables in shared memory.  The floating-point part uses numpy float64 scalars in the stated order and takes
the same k log2 k table as an argument, so that the two entropy sums can be held to the bit as well."""
import numpy as np

OK, MASKED, BAD_META, BAD_COUNTS = range(4)
TICKS_PER_BAR = {627: 1920, 628: 1440, 629: 1440, 630: 2880}   # 480 ticks a beat times 4, 3, 3, 6 beats (4/4, 3/4, 6/8, 12/8)
SLOT = 120                                                     # a sixteenth note


def entropy(counts, xlog2x):
    """H = (xlog2x[N] - S) / N for twelve integer counts with sum N > 0; every operation a float64 operation of its own"""
    N = sum(counts)
    assert N > 0 and len(counts) == 12
    S = np.float64(xlog2x[counts[0]]) + np.float64(xlog2x[counts[1]])
    for p in range(2, 12):
        S = S + np.float64(xlog2x[counts[p]])
    return (np.float64(xlog2x[N]) - S) / np.float64(N)


def row_counts(notes, meta, xlog2x, valid=True, max_bars=64, max_notes=None, n=None):
    """one row -> (counts [16], entropy (h1 sum, h4 sum) as float64, bars [max_bars][16], status).  notes: rows of (start, end, pitch,
    velocity); n: the count the row claims (default: the list's length); a row that is not OK has zeros everywhere."""
    n = len(notes) if n is None else int(n)
    zero = ([0] * 16, (np.float64(0), np.float64(0)), [[0] * 16 for _ in range(max_bars)])
    if not valid:
        return zero + (MASKED,)
    key, ts = int(meta[1]), int(meta[2])
    if not (602 <= key <= 625 and 627 <= ts <= 630):
        return zero + (BAD_META,)
    if not 0 <= n <= (len(notes) if max_notes is None else max_notes):
        return zero + (BAD_COUNTS,)
    tpb = TICKS_PER_BAR[ts]
    Q = tpb // SLOT
    per_bar = [dict(n=0, hist=[0] * 12, slots=set(), pitches=[]) for _ in range(max_bars)]
    counted, skipped, pitches = 0, 0, set()
    for j in range(n):
        start, pitch = int(notes[j][0]), int(notes[j][2])
        if start < 0 or start // tpb >= max_bars or not 0 <= pitch <= 127:
            skipped += 1
            continue
        bar = per_bar[start // tpb]
        bar["n"] += 1
        bar["hist"][pitch % 12] += 1
        bar["slots"].add((start - (start // tpb) * tpb) // SLOT)
        bar["pitches"].append(pitch)
        pitches.add(pitch)
        counted += 1
    with_notes = [k for k in range(max_bars) if per_bar[k]["n"]]
    used = 1 + max(with_notes) if with_notes else 0
    masks = [sum(1 << s for s in bar["slots"]) for bar in per_bar]
    diff = 0
    for k in range(used):
        for j in range(k):
            diff += bin(masks[j] ^ masks[k]).count("1")
    h1, w1 = np.float64(0), 0
    for k in range(used):
        if per_bar[k]["n"]:
            h1 = h1 + entropy(per_bar[k]["hist"], xlog2x)
            w1 += 1
    h4, w4 = np.float64(0), 0
    for k in range(used - 3):
        four = [sum(per_bar[k + i]["hist"][p] for i in range(4)) for p in range(12)]
        if sum(four):
            h4 = h4 + entropy(four, xlog2x)
            w4 += 1
    counts = [counted, skipped, used, len(with_notes), len({p % 12 for p in pitches}), len(pitches), min(pitches, default=-1),
              max(pitches, default=-1), sum(len(bar["slots"]) for bar in per_bar), used * (used - 1) // 2, diff, Q, w1, w4, 0, 0]
    bars = [[bar["n"], masks[k], min(bar["pitches"], default=-1), max(bar["pitches"], default=-1)] + bar["hist"] for k, bar in enumerate(per_bar)]
    return counts, (h1, h4), bars, OK


def batch_counts(notes, counts3, meta, xlog2x, valid=None, max_bars=64):
    """[B, max_notes, 4], [B, 3], [B, 11] arrays -> dict of arrays as mhm_structure_counts fills them"""
    B, max_notes = len(notes), notes.shape[1]
    rows = []
    for b in range(B):
        n = int(counts3[b][0])
        ok = 0 <= n <= max_notes
        rows.append(row_counts(notes[b][:n].tolist() if ok else [], meta[b], xlog2x, True if valid is None else bool(valid[b]), max_bars,
                               max_notes, n))
    return dict(counts=np.array([r[0] for r in rows], np.int32).reshape(B, 16), entropy=np.array([r[1] for r in rows], np.float64).reshape(B, 2),
                bars=np.array([r[2] for r in rows], np.int32).reshape(B, max_bars, 16), status=np.array([r[3] for r in rows], np.int32))


def gs(counts):
    """the groove similarity of a row from its counts, or None without a pair of bars"""
    return 1.0 - counts[10] / (counts[11] * counts[9]) if counts[9] else None


class Totals:
    """evaluation.StructureTotals without a device: Python ints, and lists of float terms that the caller sums as it likes"""

    def __init__(self):
        self.ints = [0] * 12
        self.h1, self.h4, self.gs = [], [], []

    def update(self, counts, entropy_):
        some = counts[0] > 0
        add = [1, int(some), counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[7] - counts[6] if some else 0,
               counts[8], counts[12], counts[13]]
        self.ints = [x + y for x, y in zip(self.ints, add)]
        self.h1.append(float(entropy_[0]))
        self.h4.append(float(entropy_[1]))
        if counts[9]:
            self.gs.append(gs(counts))

    def vector(self):
        import math
        return [float(x) for x in self.ints] + [math.fsum(self.h1), math.fsum(self.h4), math.fsum(self.gs), float(len(self.gs))]
