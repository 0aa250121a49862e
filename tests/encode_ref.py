"""Numpy / plain-Python restatement of the notes -> token encode path, the model the device kernels of csrc/encode.hip are
compared with, plus a seeded generator of rows.

Restated (reference sites): EventSequenceEncoder.encode (commu/preprocessor/encoder/encoder.py:21-69), extract_events /
read_items / group_items / item2event / insert_chord_on_event / detect_chord (encoder_utils.py:184-368), the chord part of
mk_remi_map / add_flat_chord2map / abstract_chord_types (:47-182), merge_and_mask (MuseDiffusion/data/preprocess.py:30-61).
tests/test_encode_cpu.py pins this file against the reference's own recorded answers (tests/golden/encode.npz); the GPU
tests then use it at batch scale.

The music arithmetic is written with numpy the way the reference writes it (linspace + argmin, searchsorted, float64 chord
positions, Python's stable sorts), NOT the way the kernel does (integer comparisons, a bitonic network with an explicit
index): agreement of the two is the check."""
import math

import numpy as np

# status codes: mirror of enum mh_encode_status (include/musehip.h) and musediffusion_amd.utils.encode_util
OK, EMPTY, NO_CHORDS, BAD_TIMEBASE, BAD_CHORDS, OVERFLOW = range(6)

EOS, BAR = 1, 2
PITCH0, VEL0, CHORD0, CHORD1, DUR0, POS0 = 3, 131, 195, 303, 304, 432
MAX_ROW = 4096        # mh_batch_max_row(): the widest `words` row
MAX_NOTES = 2048      # mh_encode_max_notes()
MAX_SLOTS = 1024      # mh_encode_max_slots()
MAX_UNITS = 4096      # measures + chord slots + notes of one row
MAX_TICKS_PER_BAR = 1 << 24
VELOCITY_BINS = np.linspace(2, 127, 64, dtype=int)

_ROOTS = ("a", "a#", "b", "c", "c#", "d", "d#", "e", "f", "f#", "g", "g#")
_QUALITIES = ("", "7", "+", "dim", "m", "m7", "m7b5", "maj7", "sus4")


def chord_vocabulary():
    """name (as written in event2word, without 'Chord_') -> token: base_event's 109 chords, then the flat-root and the
    abstracted-type aliases.  Keys keep the reference's spelling ('mM7' with a capital M: a lowercased name never finds it)."""
    v = {}
    for i, r in enumerate(_ROOTS):
        for j, q in enumerate(_QUALITIES):
            v[r + q] = CHORD0 + 9 * i + j
    v["NN"] = CHORD1
    to_base = {"": "", "maj": "", "6": "", "maj7": "maj7", "add2": "maj7", "sus2": "maj7", "7": "7", "dim": "dim", "dim7": "dim",
               "+": "+", "m": "m", "m6": "m", "mM7": "m", "m7": "m7", "madd2": "m7", "sus4": "sus4", "7sus4": "sus4", "m7b5": "m7b5"}
    for flat in ("ab", "bb", "db", "eb", "gb"):                 # add_flat_chord2map: the root a semitone below, sharpened
        sharp = "g#" if flat == "ab" else chr(ord(flat[0]) - 1) + "#"
        for scale, base in to_base.items():
            v[flat + scale] = v[sharp + base]
    abstract = {"7sus4": "sus4", "m6": "m", "sus2": "maj7", "add2": "maj7", "6": "", "dim7": "dim", "madd2": "m7", "mM7": "m7"}
    for root in "abcdefg":                                       # abstract_chord_types: natural roots only
        for scale, base in abstract.items():
            v[root + scale] = v[root + base]
    return v


CHORD_VOCABULARY = chord_vocabulary()


def chord_slots(names):
    """the host's string work: chord names, one per slot -> int32 [n, 2] = (name id, token).  Equal ids <=> equal lowercased
    full names (detect_chord compares the whole string); token = event2word of the name cut at '/' and '(' or -1 (the "OOV" print)"""
    ids, out = {}, []
    for name in names:
        low = str(name).lower()
        out.append((ids.setdefault(low, len(ids)), CHORD_VOCABULARY.get(low.split("/")[0].split("(")[0], -1)))
    return np.array(out, np.int32).reshape(-1, 2)


def timebase(tpb, num, den):
    """-> (ticks_per_bar, chords_per_bar) as encoder.py:30-31 and encoder_utils.py:201, :357 compute them, or None where the
    reference divides by zero (or, ours, where the numbers leave the range the kernel works in)"""
    if tpb <= 0 or num <= 0 or den <= 0:
        return None
    x = tpb * (num / den * 4)
    if not x < MAX_TICKS_PER_BAR + 1:
        return None
    T = int(x)
    if T < 128 or T > MAX_TICKS_PER_BAR:
        return None
    cpb = int(T / tpb) * 2
    if cpb <= 0:
        return None
    return T, cpb


def note_words(start, end, pitch, vel, bar_st, T):
    """item2event for one note -> (the four words, -1 = dropped; oov lines)"""
    flags = np.linspace(bar_st, bar_st + T, 128, endpoint=False)
    pos = int(np.argmin(abs(flags - start)))
    oov = 0
    vi = int(np.searchsorted(VELOCITY_BINS, vel, side="right")) - 1
    if 0 <= vi <= 63:
        wv = VEL0 + vi
    else:
        wv, oov = VEL0 + 63, oov + 1
    if 0 <= pitch <= 127:
        wp = PITCH0 + pitch
    else:
        wp, oov = -1, oov + 1
    step = int(T / 128)
    bins = np.arange(step, T + 1, step, dtype=int)
    di = int(np.argmin(abs(bins - (end - start))))
    wd = DUR0 + di if di <= 127 else DUR0 + 127               # an OOV duration is replaced silently
    return [POS0 + pos, wv, wp, wd], oov


def encode_events(notes, n_notes, params, slots, n_slots, ld, max_notes=None, max_slots=None):
    """one row -> (words list ending in EOS ([] unless OK), (events, oov lines), status).  notes [*, 4] = (start, end, pitch,
    velocity); params = (ticks_per_beat, numerator, denominator, ceil(num_measures), is_incomplete_measure); slots [*, 2]"""
    notes = np.asarray(notes, np.int64).reshape(-1, 4)
    slots = np.asarray(slots, np.int64).reshape(-1, 2)
    max_notes = len(notes) if max_notes is None else max_notes
    max_slots = len(slots) if max_slots is None else max_slots
    tpb, num, den, NM, inc = (int(x) for x in params)
    inc = 1 if inc else 0
    fail = lambda st: ([], (0, 0), st)  # noqa: E731
    tb = timebase(tpb, num, den)
    if tb is None:
        return fail(BAD_TIMEBASE)
    T, cpb = tb
    if n_notes <= 0:
        return fail(EMPTY)
    if n_slots <= 0:
        return fail(NO_CHORDS)
    if n_notes > max_notes or n_notes > MAX_NOTES or n_slots > max_slots or n_slots > MAX_SLOTS:
        return fail(OVERFLOW)
    if n_slots % cpb:
        return fail(BAD_CHORDS)
    NM = max(NM, 0)
    if NM + n_slots + n_notes > MAX_UNITS:
        return fail(OVERFLOW)
    # read_items: sort by (start, pitch), then two stable sorts by start
    items = [tuple(int(x) for x in notes[k]) for k in range(n_notes)]
    items.sort(key=lambda x: (x[0], x[2]))
    items.sort(key=lambda x: x[0])
    max_time = items[-1][1]
    # group_items: downbeats = np.arange(0, max_time + T, T), one group per pair of neighbours; the items are in start order, so walking
    # the groups and the items of each is walking the items that start in [0, last downbeat) (the array itself can have 2^31 / T
    # entries for a hostile end, so only its length is computed)
    n_downbeats = max(0, -((-(max_time + T)) // T))
    events = []                                                 # (time, words)
    n_events = oov = 0
    for (start, end, pitch, vel) in items:
        if n_downbeats >= 2 and 0 <= start < (n_downbeats - 1) * T:
            w, o = note_words(start, end, pitch, vel, (start // T) * T, T)
            events.append((start, w))
            n_events, oov = n_events + 4, oov + o
    # detect_chord + insert_chord_on_event
    chord_idx, chord_tok = [], []
    last = None
    for s in range(n_slots):
        bar, c = divmod(s, cpb)
        if c == 0 or int(slots[s, 0]) != last:
            chord_idx.append(bar + c / cpb)
            chord_tok.append(int(slots[s, 1]))
            last = int(slots[s, 0])
    start_time = T * inc
    chord_events = []
    for i in range(NM):
        chord_events.append((i * T, [BAR]))
        n_events += 1
        while chord_idx and chord_idx[0] < i + 1 - inc:
            p = chord_idx.pop(0)
            tok = chord_tok.pop(0)
            t = int(p * T + start_time)
            v = int((p - i + inc) * 128) + 1
            wpos = POS0 + v - 1 if 1 <= v <= 128 else -1
            wch = tok if CHORD0 <= tok <= CHORD1 else -1
            oov += (wpos < 0) + (wch < 0)
            chord_events.append((t, [wpos, wch]))
            n_events += 2
    merged = chord_events + events
    merged.sort(key=lambda e: e[0])
    words = [w for _, ws in merged for w in ws if w >= 0] + [EOS]
    if len(words) > ld:
        return fail(OVERFLOW)
    return words, (n_events, oov), OK


def merge_row(src, trg):
    """preprocess.py:36-56 for one row -> (input_ids, input_mask) lists; the index arithmetic is numpy's own"""
    src, trg = np.asarray(src, np.int64), np.asarray(trg, np.int64)
    chord = np.logical_and(195 <= trg, trg <= 303)
    idx = np.repeat(np.where(chord)[0], 2)
    idx[::2] -= 1
    keep = np.ones_like(trg, dtype="?")
    keep[idx] = False
    src = np.concatenate([src, trg[idx]])
    trg = trg[keep]
    return [*src.tolist(), 1, *trg.tolist()], [0] * (len(src) + 1) + [1] * len(trg)


# ---------------------------------------------------------------------------------------------------------------- generator
TIME_SIGNATURES = ((4, 4), (3, 4), (6, 8), (12, 8))
_NAMES = ("C", "Am", "F", "G7", "Dm7", "Ebmaj7", "Bbsus2", "F#dim", "G/B", "Asus4(9)", "E+", "Bm7b5", "Abm6", "Dadd2", "X9", "C#m6")


def make_item(g, kind="clean", n_notes=None, tpb=None, ts=None, measures=None):
    """-> dict(notes [k, 4], params (5,), names list): one row of plausible music with the perturbation `kind` names"""
    num, den = TIME_SIGNATURES[int(g.integers(0, 4))] if ts is None else ts
    tpb = int(g.choice([480, 96, 220, 384])) if tpb is None else tpb
    T, cpb = timebase(tpb, num, den)
    M = int(g.choice([4, 8, 16])) if measures is None else measures
    inc = int(g.integers(0, 2))
    n = int(g.integers(8, 200)) if n_notes is None else n_notes
    start = np.sort(g.integers(0, (M + inc) * T, n))
    if g.integers(0, 2):
        start = (start // (T // 16)) * (T // 16)               # quantised: equal starts, bar boundaries, position ties
    dur = g.integers(1, T, n)
    notes = np.stack([start, start + dur, g.integers(20, 110, n), g.integers(1, 128, n)], 1)
    notes = notes[g.permutation(n)]                           # input order is not time order
    names = []
    for _ in range(M):
        bar = [str(g.choice(_NAMES))]
        for _ in range(cpb - 1):
            bar.append(str(g.choice(_NAMES)) if g.random() < 0.25 else bar[-1])
        names += bar
    params = [tpb, num, den, M + inc, inc]
    if kind == "empty":
        notes = notes[:0]
    elif kind == "no_chords":
        names = []
    elif kind == "bad_timebase":
        params[0] = int(g.choice([0, 7, 31]))
    elif kind == "bad_chords":
        names = names[:-1]
    elif kind == "hostile_notes":
        k = g.integers(0, n, 4)
        notes[k[0], 2], notes[k[1], 2], notes[k[2], 3], notes[k[3], 0] = -1, 128, 0, -5
        notes[int(np.lexsort((notes[:, 2], notes[:, 0]))[-1]), 1] = (M // 2) * T   # the last sorted note ends early: later notes are lost
    return dict(notes=notes.astype(np.int32).reshape(-1, 4), params=np.array(params, np.int32), names=names)


BATCH_KINDS = ("clean",) * 40 + ("hostile_notes",) * 8 + ("empty",) * 4 + ("no_chords",) * 4 + ("bad_timebase",) * 4 + ("bad_chords",) * 4


def pack(items, max_notes=None, max_slots=None):
    """items -> the kernel's padded inputs: notes [B, max_notes, 4], n_notes [B], params [B, 5], slots [B, max_slots, 2], n_slots [B]"""
    B = len(items)
    sl = [chord_slots(it["names"]) for it in items]
    max_notes = max(1, max(len(it["notes"]) for it in items)) if max_notes is None else max_notes
    max_slots = max(1, max(len(s) for s in sl)) if max_slots is None else max_slots
    notes, slots = np.zeros((B, max_notes, 4), np.int32), np.zeros((B, max_slots, 2), np.int32)
    for b, it in enumerate(items):
        notes[b, :len(it["notes"])] = it["notes"]
        slots[b, :len(sl[b])] = sl[b]
    return dict(notes=notes, n_notes=np.array([len(it["notes"]) for it in items], np.int32),
                params=np.stack([it["params"] for it in items]).astype(np.int32), slots=slots,
                n_slots=np.array([len(s) for s in sl], np.int32))


def make_batch(seed, kinds=BATCH_KINDS):
    g = np.random.default_rng(seed)
    kinds = [kinds[i] for i in g.permutation(len(kinds))]
    return [make_item(g, k) for k in kinds], kinds


def bench_items(B=512, seed=9):
    """the rows tools/batch_bench.py and tools/make_golden_encode.py --time-reference time: about 500 notes over 16 measures each"""
    g = np.random.default_rng(seed)
    return [make_item(g, "clean", n_notes=int(g.integers(450, 551)), measures=16) for _ in range(B)]


def encode_rows(p, ld):
    """the restatement over pack()'s arrays -> list of (words, counts, status)"""
    B, max_notes, max_slots = len(p["n_notes"]), p["notes"].shape[1], p["slots"].shape[1]
    return [encode_events(p["notes"][b], int(p["n_notes"][b]), p["params"][b], p["slots"][b], int(p["n_slots"][b]), ld, max_notes, max_slots)
            for b in range(B)]
