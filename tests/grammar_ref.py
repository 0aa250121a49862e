"""Numpy / plain-Python restatement of the grammar-constrained rounding (include/musehip_grammar.h, csrc/grammar.hip), the model the
two kernels are compared with, plus the brute-force enumeration it is itself checked against (tests/test_grammar_cpu.py).

`class_winners` works in float64 (the kernel's fp32 scores are held to a bound around it); `constrain_row` steps the automaton in
fp32 in the order the header defines, so that its tokens, status, counts and path score are the kernel's bit for bit on the same
tables.  The pass loops over positions; every line of a step is elementwise over the Bar count k, as the kernel's lanes are."""
import numpy as np

# mirror of enum mhg_class, enum mhg_status and enum mhg_bars
PAD, EOS, BAR, PITCH, VELOCITY, DURATION, POSITION, ANY = range(8)
OK, BAD_MASK, NO_CHORDS, TOO_MANY_BARS, BAD_BOUNDS, NO_ROOM, NONFINITE = range(7)
BARS_EXACT, BARS_DECODABLE = 0, 1
STATUS_NAMES = ("OK", "BAD_MASK", "NO_CHORDS", "TOO_MANY_BARS", "BAD_BOUNDS", "NO_ROOM", "NONFINITE")
MAX_K = 63

# the ComMU vocabulary as [lo, hi) per class (mhg_note_classes)
NOTE_CLASSES = ((0, 1), (1, 2), (2, 3), (3, 131), (131, 195), (304, 432), (432, 560))

A0, B0, V, P, D, END = range(6)


# ------------------------------------------------------------------------------------------------------------------ class winners
def scores64(x, table, aux, mode):
    """the [n, V] scores in float64: mode 1 x.W + b, mode 2 -sqrt(max((aux + |x|^2) - 2 x.W, 0))"""
    x, table, aux = (np.asarray(a, np.float64) for a in (x, table, aux))
    dots = x @ table.T
    if mode == 1:
        return dots + aux[None, :]
    return -np.sqrt(np.maximum((aux[None, :] + (x * x).sum(1)[:, None]) - 2.0 * dots, 0.0))


def class_winners(scores, classes):
    """scores [n, V] -> (cls_score [n, 8], cls_idx [n, 8]): per class the maximum and its first index over the part of [lo, hi) inside
    [0, V); slot 7 the whole vocabulary.  A class without a token, or whose scores are all -inf, gives (-inf, -1); slot 7 (-inf, 0)."""
    n, Vn = scores.shape
    cs = np.full((n, 8), -np.inf, scores.dtype)
    ci = np.full((n, 8), -1, np.int32)
    ci[:, ANY] = 0
    ranges = [(max(int(lo), 0), min(int(hi), Vn)) for lo, hi in classes] + [(0, Vn)]
    for c, (lo, hi) in enumerate(ranges):
        if hi <= lo:
            continue
        part = scores[:, lo:hi]
        best = part.argmax(1)
        val = part[np.arange(n), best]
        hit = val > -np.inf
        cs[hit, c] = val[hit]
        ci[hit, c] = (lo + best[hit]).astype(np.int32)
    return cs, ci


# ------------------------------------------------------------------------------------------------------------------ row Viterbi
def row_bounds(ids, mask, policy=BARS_EXACT, lo=None, hi=None):
    """-> (status, len_meta, lo, hi): the part of the status that is decided before the region is read"""
    L = len(ids)
    len_meta = L - int(np.asarray(mask, np.int64).sum())
    if len_meta < 0 or len_meta >= L:
        return BAD_MASK, 0, 0, 0
    if lo is None:
        n432 = sum(1 for t in list(ids)[11:len_meta - 1] if int(t) == 432)    # len_meta 0: the -1 counts from the end, as restore_chord
        if n432 == 0:
            return NO_CHORDS, len_meta, 0, 0
        lo, hi = (0, n432 + 1) if policy == BARS_DECODABLE else (n432, n432)
    lo, hi = int(lo), int(hi)
    if hi > MAX_K:
        return TOO_MANY_BARS, len_meta, lo, hi
    if lo < 0 or lo > hi:
        return BAD_BOUNDS, len_meta, lo, hi
    return OK, len_meta, lo, hi


def viterbi(cs, ci, lo, hi):
    """cs / ci [n, 8]: the region's tables.  -> (status, classes [n] or None, path score fp32, (bars, notes, through_eos))"""
    n = len(cs)
    f = np.float32
    cs = np.asarray(cs, f)
    if not np.all(cs[:, :7] < np.inf):                               # NaN or +inf in a used slot
        return NONFINITE, None, f(0), (0, 0, 0)
    K = hi + 1
    reach = np.zeros((6, K), bool)
    score = np.zeros((6, K), f)
    reach[A0, 0] = True
    dV, dB, dE = (np.zeros((n, K), bool) for _ in range(3))

    def up(a):
        """the value at k - 1; nothing below k = 0"""
        return np.concatenate([np.zeros(1, a.dtype), a[:-1]])

    def meet(r1, s1, r2, s2):
        """first-listed (r1, s1) unless the later one is reachable and the first is not, or strictly greater"""
        second = r2 & (~r1 | (s2 > s1))
        return r1 | r2, np.where(second, s2, s1), second

    for t in range(n):                                               # every line below is elementwise over k, in fp32
        ok = ci[t, :7] >= 0
        s = cs[t]
        nr, ns = np.zeros_like(reach), np.zeros_like(score)
        # A0 <- A0 (k - 1) on BAR
        nr[A0], ns[A0] = up(reach[A0]) & ok[BAR], up(score[A0]) + s[BAR]
        # V <- A0 | B0 on POSITION
        nr[V], ns[V], dV[t] = meet(reach[A0] & ok[POSITION], score[A0] + s[POSITION], reach[B0] & ok[POSITION], score[B0] + s[POSITION])
        nr[P], ns[P] = reach[V] & ok[VELOCITY], score[V] + s[VELOCITY]
        nr[D], ns[D] = reach[P] & ok[PITCH], score[P] + s[PITCH]
        # B0 <- D on DURATION | B0 (k - 1) on BAR
        nr[B0], ns[B0], dB[t] = meet(reach[D] & ok[DURATION], score[D] + s[DURATION], up(reach[B0]) & ok[BAR], up(score[B0]) + s[BAR])
        # END <- B0 on EOS | END on PAD
        nr[END], ns[END], dE[t] = meet(reach[B0] & ok[EOS], score[B0] + s[EOS], reach[END] & ok[PAD], score[END] + s[PAD])
        assert ns.dtype == f
        reach, score = nr, ns
    best = -1
    for k in range(lo, K):
        if reach[END, k] and (best < 0 or score[END, k] > score[END, best]):
            best = k
    if best < 0:
        return NO_ROOM, None, f(0), (0, 0, 0)
    classes = np.zeros(n, np.int64)
    state, k, notes, through = END, best, 0, 0
    for t in range(n - 1, -1, -1):
        if state == END:
            if dE[t, k]:
                c = PAD
            else:
                c, state, through = EOS, B0, t + 1
        elif state == B0:
            if dB[t, k]:
                c, k = BAR, k - 1
            else:
                c, state, notes = DURATION, D, notes + 1
        elif state == D:
            c, state = PITCH, P
        elif state == P:
            c, state = VELOCITY, V
        elif state == V:
            c, state = POSITION, (B0 if dV[t, k] else A0)
        else:
            c, k = BAR, k - 1
        classes[t] = c
    assert state == A0 and k == 0
    return OK, classes, score[END, best], (best, notes, through)


def constrain_row(cs, ci, ids, mask, policy=BARS_EXACT, lo=None, hi=None):
    """cs / ci [L, 8] -> dict(tokens [L] int32, status, path_score fp32, counts (3,))"""
    L = len(ids)
    ci = np.asarray(ci, np.int32)
    st, len_meta, lo, hi = row_bounds(ids, mask, policy, lo, hi)
    out = dict(tokens=ci[:, ANY].copy(), status=st, path_score=np.float32(0), counts=(0, 0, 0))
    if st != OK:
        return out
    st, classes, total, counts = viterbi(np.asarray(cs)[len_meta:], ci[len_meta:], lo, hi)
    out["status"] = st
    if st == OK:
        out["tokens"][len_meta:] = ci[np.arange(len_meta, L), classes]
        out["path_score"], out["counts"] = np.float32(total), counts
    return out


def constrain_rows(cs, ci, ids, mask, policy=BARS_EXACT, lo=None, hi=None):
    """cs / ci [B, L, 8], ids / mask [B, L] -> dict of arrays (tokens [B, L], status [B], path_score [B], counts [B, 3])"""
    B = len(ids)
    rows = [constrain_row(cs[b], ci[b], ids[b], mask[b], policy, None if lo is None else lo[b], None if hi is None else hi[b])
            for b in range(B)]
    return dict(tokens=np.stack([r["tokens"] for r in rows]).astype(np.int32), status=np.array([r["status"] for r in rows], np.int32),
                path_score=np.array([r["path_score"] for r in rows], np.float32),
                counts=np.array([r["counts"] for r in rows], np.int32).reshape(B, 3))


# ------------------------------------------------------------------------------------------------------------------ brute force
def accepted_strings(n, lo, hi):
    """every class string of length n the grammar accepts with lo <= Bars <= hi (small n only)"""
    out = []

    def events(prefix, bars, notes):
        room = n - len(prefix)
        if notes >= 1 and lo <= bars <= hi and room >= 1:
            out.append(prefix + [EOS] + [PAD] * (room - 1))
        if room >= 2 and bars < hi:
            events(prefix + [BAR], bars + 1, notes)
        if room >= 5:
            events(prefix + [POSITION, VELOCITY, PITCH, DURATION], bars, notes + 1)

    events([], 0, 0)
    return out


def brute_force(cs, lo, hi):
    """-> (best strings as tuples, best float64 score) over every accepted string; ([], None) when there is none"""
    n = len(cs)
    best, which = None, []
    for s in accepted_strings(n, lo, hi):
        total = float(sum(float(cs[t, c]) for t, c in enumerate(s)))
        if best is None or total > best:
            best, which = total, [tuple(s)]
        elif total == best:
            which.append(tuple(s))
    return which, best
