"""Numpy / plain-Python restatement of the token -> notes decode path, the model the device kernels of csrc/decode.hip are
compared with, plus a seeded generator of ComMU-shaped rows with perturbations.

Restated (reference sites): SequenceToMidi.split_meta_midi / remove_padding / restore_chord / validate_once /
validate_rigidly (utils/decode_util.py:73-199), EventSequenceEncoder.decode (commu/preprocessor/encoder/encoder.py:71-97),
word_to_event / write_midi (encoder_utils.py:370-497).  tests/test_decode_cpu.py pins this file against the reference's own
recorded answers (tests/golden/decode.npz); the GPU tests then use it at batch scale.

Everything is written with explicit indices (no numpy slicing tricks), the way the kernels do it, so that the fixture checks
the index arithmetic and not numpy's."""
import numpy as np

# status codes: mirror of enum mh_decode_status (include/musehip.h) and musediffusion_amd.utils.decode_util
OK, NO_EOS, RESTORE_FAILED, ONCE_FAILED, STRICT_FAILED, REF_INDEXERROR, BAD_META, OVERFLOW = range(8)

EOS, BAR = 1, 2
PITCH0, VEL0, CHORD0, DUR0, POS0, BPM0, KEY0, TS0 = 3, 131, 195, 304, 432, 560, 601, 626
BEATS = (4, 3, 3, 6)                                    # int(num / den * 4) of 4/4, 3/4, 6/8, 12/8 (tokens 627..630)
VELOCITY = [2 + (125 * k) // 63 for k in range(64)]     # np.linspace(2, 127, 64, dtype=int)
MAX_ROW = 4096                                          # mh_batch_max_row()


def split_and_restore(seq, mask, ld_out):
    """-> (restored list, meta list of 11 (0-padded), status, branch 0 / 1 / 2 or -1)"""
    seq = [int(t) for t in seq]
    L = len(seq)
    len_meta = L - int(np.asarray(mask, dtype=np.int64).sum())
    meta11 = [0] * 11
    if len_meta < 0 or len_meta > L:                    # ours: a mask that is no 0/1 mask
        return [], meta11, BAD_META, -1
    meta_len = len_meta - 1 if len_meta >= 1 else L - 1   # seq[:len_meta - 1]: -1 counts from the end
    for k in range(min(11, meta_len)):
        meta11[k] = seq[k]
    ci = seq[11:meta_len]                               # the chord part
    C = len(ci)
    eos = -1
    for j in range(len_meta, L):
        if seq[j] == EOS:
            eos = j
            break
    if eos < 0:
        return [], meta11, NO_EOS, -1
    s = seq[len_meta:eos + 1]
    n = len(s)
    bars = [j for j in range(n) if s[j] == BAR]
    nb = len(bars)
    n432 = sum(1 for t in ci if t == 432)
    if nb == n432:
        branch = 0
        if nb == 0:
            return [], meta11, REF_INDEXERROR, branch
        bc = 0
    elif nb == n432 + 1:
        branch = 1
        if nb < 2:
            return [], meta11, REF_INDEXERROR, branch
        bc = 1
    elif nb < n432:
        branch = 2
        diff = n432 - nb
        if n + diff > MAX_ROW:                          # ours: only a len_meta of 0 gets here (else n + diff <= L)
            return [], meta11, OVERFLOW, branch
        last = s[n - 1]
        s = s[:n - 1] + [BAR] * diff + [last]
        bars = bars + list(range(n - 1, n - 1 + diff))
        n += diff
        nb = n432
        bc = 0
    else:
        return [], meta11, RESTORE_FAILED, 3
    last_idx = bars[bc]
    out = s[:last_idx + 1] + ci[:2]
    for i in range(2, C, 2):
        pair = ci[i:i + 2]
        if ci[i] == 432:
            if bc + 1 >= nb:
                return [], meta11, REF_INDEXERROR, branch
            stop = bars[bc + 1] + 1
            if stop > last_idx + 1:
                out += s[last_idx + 1:stop]
            out += pair
            bc += 1
            last_idx = bars[bc]
        else:
            lo = bars[bc]
            hi = bars[bc + 1] if bc != nb - 1 else n
            p = -1
            for j in range(lo + 1, hi):
                if 432 <= s[j] < ci[i]:
                    p = j
            if p >= 0:
                stop = min(p + 4, n)
                if stop > last_idx + 1:
                    out += s[last_idx + 1:stop]
                last_idx = p + 3
            out += pair
    if last_idx + 1 < n:
        out += s[last_idx + 1:]
    if len(out) > ld_out:
        return [], meta11, OVERFLOW, branch
    return out, meta11, OK, branch


def validate_once(seq):
    n = len(seq)
    for i in range(0, n - 2):
        prev = seq[i - 1] if i > 0 else seq[n - 1]
        if VEL0 <= seq[i] < CHORD0 and POS0 <= prev < BPM0 and PITCH0 <= seq[i + 1] < VEL0 and DUR0 <= seq[i + 2] < POS0:
            return True
    return False


def validate_rigidly(seq):
    """1 pass, 0 fail, -2 where the reference indexes past the end"""
    i, n = 0, len(seq)
    while True:
        if i >= n:
            return 0
        t = seq[i]
        if t == EOS:
            return 1
        if t == BAR:
            i += 1
            continue
        if not (POS0 <= t < BPM0):
            return 0
        if i + 1 >= n:
            return -2
        t1 = seq[i + 1]
        if VEL0 <= t1 < CHORD0:
            if i + 3 >= n:                              # all([...]) builds the whole list first: seq[i + 3] is always read
                return -2
            if PITCH0 <= seq[i + 2] < VEL0 and DUR0 <= seq[i + 3] < POS0:
                i += 4
                continue
            return 0
        if CHORD0 <= t1 < DUR0:
            i += 2
            continue
        return 0


def decode_events(restored, meta11, max_notes, max_chords):
    """-> (notes [k, 4], chords [k, 2], n_oov, status OK | OVERFLOW); meta11 must have passed meta_ok"""
    comp, oov = [], 0
    for t in restored:
        if 2 <= t <= 559:
            comp.append(t)
        elif t != EOS:
            oov += 1
    tpb = 480 * BEATS[meta11[2] - 627]
    dstep = tpb // 128
    notes, chords = [], []
    bar = 0
    m = len(comp)
    for i in range(m - 3):
        t = comp[i]
        if t == BAR and i > 0:
            bar += 1
        elif POS0 <= t < BPM0:
            t1, t2, t3 = comp[i + 1], comp[i + 2], comp[i + 3]
            start = bar * tpb + ((t - POS0) * tpb) // 128
            if VEL0 <= t1 < CHORD0 and PITCH0 <= t2 < VEL0 and DUR0 <= t3 < POS0:
                notes.append((start, start + (t3 - DUR0 + 1) * dstep, t2 - PITCH0, VELOCITY[t1 - VEL0]))
            elif CHORD0 <= t1 < DUR0:
                chords.append((start, t1))
    st = OVERFLOW if len(notes) > max_notes or len(chords) > max_chords else OK
    return (np.array(notes, np.int32).reshape(-1, 4), np.array(chords, np.int32).reshape(-1, 2), oov, st)


def meta_ok(meta11):
    """a meta of fewer than 11 tokens has an empty chord part and never survives restore_chord: the three slots are the meta's own"""
    return 561 <= meta11[0] <= 600 and 602 <= meta11[1] <= 625 and 627 <= meta11[2] <= 630


def decode_row(seq, mask, ld_out, max_notes, max_chords, strict=False):
    """The whole path for one row -> dict(status, restored, meta, notes, chords, counts, oov, branch); the order of the checks is
    the order in which the reference raises (SequenceToMidi.decode).  counts = (notes, chords, oov) as the kernel reports them:
    the true totals of every row that reaches the event pass (OVERFLOW rows too), zero otherwise."""
    restored, meta11, st, branch = split_and_restore(seq, mask, ld_out)
    r = dict(status=st, restored=np.array(restored, np.int32), meta=np.array(meta11, np.int32), branch=branch,
             notes=np.zeros((0, 4), np.int32), chords=np.zeros((0, 2), np.int32), oov=0, counts=(0, 0, 0))
    if st != OK:
        return r
    if not validate_once(restored):
        r["status"] = ONCE_FAILED
        return r
    if strict:
        v = validate_rigidly(restored)
        if v != 1:
            r["status"] = REF_INDEXERROR if v == -2 else STRICT_FAILED
            return r
    if not meta_ok(meta11):
        r["status"] = BAD_META
        return r
    notes, chords, oov, st = decode_events(restored, meta11, max_notes, max_chords)
    r["status"], r["oov"], r["counts"] = st, oov, (len(notes), len(chords), oov)
    if st == OK:
        r["notes"], r["chords"] = notes, chords
    return r


def decode_rows(tokens, masks, ld_out, max_notes, max_chords, strict=False):
    return [decode_row(tokens[b], masks[b], ld_out, max_notes, max_chords, strict) for b in range(len(tokens))]


# ---------------------------------------------------------------------------------------------------------------- generator
def make_meta(g, n_bars, changes, ts=None):
    """11 meta tokens + the chord part of MetaToSequence.encode_chord: per bar 432, chord, then (432 + 16 i, chord) per change"""
    meta = [int(g.integers(561, 601)), int(g.integers(602, 626)), int(ts if ts is not None else g.integers(627, 631)),
            int(g.integers(631, 638)), int(g.integers(638, 641)), int(g.integers(641, 650)), int(g.integers(650, 653)),
            int(g.integers(654, 680)), int(g.integers(690, 719)), int(g.integers(719, 726)), int(g.integers(726, 729))]
    chord = []
    for _ in range(n_bars):
        chord += [432, int(g.integers(195, 304))]
        for i in sorted(g.choice(np.arange(1, 8), size=int(g.integers(0, changes + 1)), replace=False)):
            chord += [432 + 16 * int(i), int(g.integers(195, 304))]
    return meta, chord


def make_notes(g, n_bars, notes_per_bar):
    """what the model is trained to emit: bars of (position, velocity, pitch, duration) with no chord events, then EOS"""
    s = []
    for _ in range(n_bars):
        s.append(BAR)
        for p in sorted(g.choice(np.arange(432, 560), size=notes_per_bar, replace=False)):
            s += [int(p), int(g.integers(131, 195)), int(g.integers(3, 131)), int(g.integers(304, 432))]
    return s + [EOS]


KINDS = ("clean", "extra_bar", "drop_bars", "two_extra_bars", "no_eos", "no_notes", "truncated", "garbage", "no_chords", "shift_mask", "bad_meta")


def make_row(g, L, kind, n_bars=None, notes_per_bar=None):
    """one [L] token row and its input mask.  `kind` names the perturbation (KINDS)."""
    n_bars = int(g.integers(4, 9)) if n_bars is None else n_bars
    npb = int(g.integers(4, 8)) if notes_per_bar is None else notes_per_bar
    meta, chord = make_meta(g, n_bars, 2)
    notes = make_notes(g, n_bars, npb)
    bar_at = [j for j, t in enumerate(notes) if t == BAR]
    if kind == "extra_bar":                                # the leading empty bar the training data often has
        notes = [BAR] + notes
    elif kind == "drop_bars":
        for j in sorted(g.choice(bar_at[1:], size=min(2, len(bar_at) - 1), replace=False), reverse=True):
            del notes[j]
    elif kind == "two_extra_bars":
        notes = [BAR, BAR] + notes
    elif kind == "no_eos":
        notes = notes[:-1]
    elif kind == "no_notes":                               # chords only: validate_once fails
        notes = [BAR] * n_bars + [EOS]
    elif kind == "truncated":                              # a note cut short before the EOS: the strict validator's trouble
        cut = int(g.integers(1, 4))
        notes = notes[:-1][:len(notes) - 1 - cut] + [EOS]
    elif kind == "garbage":
        for j in g.choice(np.arange(1, len(notes) - 1), size=3, replace=False):
            notes[int(j)] = int(g.choice([0, 560, 600, 728, 3, 200]))
    elif kind == "no_chords":                              # the chord part is missing and the notes hold one bar: IndexError
        chord = []
        notes = make_notes(g, 1, npb)
    elif kind == "bad_meta":                               # a time-signature or key token outside its range
        k = int(g.integers(1, 3))
        meta[k] = int(g.choice([601, 626] if k == 1 else [626, 631]))
    pre = meta + chord
    row = pre + [0] + notes
    assert len(row) <= L, (len(row), L)
    row = row + [0] * (L - len(row))
    mask = [0] * (len(pre) + 1) + [1] * (L - len(pre) - 1)
    if kind == "shift_mask":                               # a mask one short / one long: the split lands one token off
        d = int(g.choice([-1, 1]))
        mask = [0] * (len(pre) + 1 + d) + [1] * (L - len(pre) - 1 - d)
    return np.array(row, np.int32), np.array(mask, np.int32)


# 96 rows: 44 that decode (through each entry branch of restore_chord), 8 of each failure, 12 that only the strict validator rejects
BATCH_KINDS = (("clean",) * 20 + ("extra_bar",) * 12 + ("drop_bars",) * 12 + ("no_eos",) * 8 + ("two_extra_bars",) * 8 +
               ("no_notes",) * 8 + ("truncated",) * 4 + ("garbage",) * 4 + ("shift_mask",) * 4 + ("no_chords",) * 8 + ("bad_meta",) * 8)


def make_batch(seed, L, kinds=BATCH_KINDS):
    """-> tokens [B, L], masks [B, L] (int32), one row per entry of `kinds`, in a seeded shuffled order"""
    g = np.random.default_rng(seed)
    kinds = [kinds[i] for i in g.permutation(len(kinds))]
    toks, masks = np.zeros((len(kinds), L), np.int32), np.zeros((len(kinds), L), np.int32)
    for b, kind in enumerate(kinds):
        toks[b], masks[b] = make_row(g, L, kind)
    return toks, masks, kinds


def make_dense_rows(g, B, L, n_bars, notes_per_bar):
    """-> tokens [B, L], masks [B, L] (int32): B clean rows of n_bars full bars with one chord each - the batch tools/ time on"""
    toks, masks = np.zeros((B, L), np.int32), np.zeros((B, L), np.int32)
    for b in range(B):
        meta, chord = make_meta(g, n_bars, 0)
        row = meta + chord + [0] + make_notes(g, n_bars, notes_per_bar)
        assert len(row) <= L, (len(row), L)
        toks[b, :len(row)] = row
        masks[b, len(meta) + len(chord) + 1:] = 1
    return toks, masks
