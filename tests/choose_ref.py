"""Plain restatement of the rules of include/musehip_choose.h, the model csrc/choose.hip is compared with bit for bit, and of
metric.fit_scores.  Written from the rules' wording and NOT the way the kernels compute: no tiles and no partial sums in pair_fit -
two rows' counted notes stand in numpy int64 columns and every pair of them is looked at; no lists of eligible candidates and no
mixed radix in choose - EVERY q in 0 .. K^T - 1 is written out in its digits, the inadmissible ones are struck, and the objective of
the others is summed term by term (in numpy columns over q, so that 2^20 combinations stay affordable; tests/test_choose_cpu.py holds
this against itertools.product).  Everything is an integer."""
import numpy as np

import interplay_ref as ir

OK, MASKED, BAD_COUNTS, BAD_SHIFT, MIXED = range(5)                      # enum mha_status
CH_OK, CH_PARTIAL, CH_EMPTY, CH_BAD_SCORE = range(4)                     # enum mhac_status
MAX_TICK, CLAMP = ir.MAX_TICK, ir.CLAMP
SCORE_MAX, WEIGHT_MAX, MAX_COMBINATIONS = 2 ** 40, 1024, 2 ** 20
DEFAULT_WEIGHTS = (0, -2, -2, 1, 1, 1, -2)


def meet(mine, theirs):
    """two lists of counted notes [k, 3] = (shifted start, shifted end, pitch) -> (ticks [7], pairs [7]) over the interval classes"""
    ticks, pairs = np.zeros(7, np.int64), np.zeros(7, np.int64)
    if not len(mine) or not len(theirs):
        return ticks, pairs
    step = max(1, (1 << 20) // len(theirs))
    for i in range(0, len(mine), step):
        x = mine[i:i + step]
        o = np.minimum(x[:, None, 1], theirs[None, :, 1]) - np.maximum(x[:, None, 0], theirs[None, :, 0])
        together = o > 0
        d = np.abs(x[:, None, 2] - theirs[None, :, 2]) % 12
        ic = np.minimum(d, 12 - d)[together]
        common = np.minimum(o[together], CLAMP)
        for c in range(7):
            pairs[c] += int((ic == c).sum())
            ticks[c] += int(common[ic == c].sum())
    return ticks, pairs


def pair_fit(notes, counts3, meta, S, T, K, valid=None, shift=None):
    """[B, max_notes, 4], [B, 3], [B, 11] arrays in the candidate layout (+ valid, shift [B] or None) -> dict of arrays as
    mhac_pair_fit fills them: ticks and pairs int64 [B, R, 7], status int32 [B]"""
    R, B = T * K, S * T * K
    max_notes = np.asarray(notes).shape[1]
    assert len(notes) == B
    n = [int(counts3[b][0]) for b in range(B)]
    s = [0 if shift is None else int(shift[b]) for b in range(B)]
    on = [True if valid is None else int(valid[b]) != 0 for b in range(B)]
    in_range = [on[b] and 0 <= n[b] <= max_notes and 0 <= s[b] <= MAX_TICK for b in range(B)]
    ticks, pairs, status = np.zeros((B, R, 7), np.int64), np.zeros((B, R, 7), np.int64), np.zeros(B, np.int32)
    lists = {}

    def counted(c):
        if c not in lists:
            lists[c] = ir.counted_notes(notes[c], n[c], s[c])
        return lists[c]

    for b in range(B):
        if not on[b]:
            status[b] = MASKED
        elif not 0 <= n[b] <= max_notes:
            status[b] = BAD_COUNTS
        elif not 0 <= s[b] <= MAX_TICK:
            status[b] = BAD_SHIFT
        if status[b]:
            continue
        song, track = b // R, b % R // K
        partners = [c for c in range(song * R, song * R + R) if c % R // K != track and in_range[c]]
        if any(int(meta[c][i]) != int(meta[b][i]) for c in partners for i in range(3)):
            status[b] = MIXED
            continue
        for c in partners:
            ticks[b, c % R], pairs[b, c % R] = meet(counted(b), counted(c))
    return dict(ticks=ticks, pairs=pairs, status=status)


def fit_scores(ticks, weights=DEFAULT_WEIGHTS):
    """ticks [S * R, R, 7] -> W int64 [S, R, R] in Python integers: the weighted sum over the classes, clamped to +-2^40"""
    ticks = np.asarray(ticks)
    BR, R = ticks.shape[0], ticks.shape[1]
    assert len(weights) == 7 and all(abs(int(w)) <= WEIGHT_MAX for w in weights) and BR % R == 0
    W = np.zeros((BR // R, R, R), np.int64)
    for b in range(BR):
        for r in range(R):
            v = sum(int(weights[c]) * int(ticks[b, r, c]) for c in range(7))
            W[b // R, b % R, r] = max(-SCORE_MAX, min(SCORE_MAX, v))
    return W


def choose(W, S, T, K, unary=None, eligible=None):
    """W [S, R, R], unary [S, R] or None, eligible [S, R] or None -> dict of arrays as mhac_choose fills them: choice int32 [S, T],
    best and first int64 [S], status int32 [S]"""
    R = T * K
    assert K ** T <= MAX_COMBINATIONS
    W = np.asarray(W, np.int64).reshape(S, R, R)
    choice, best, first = np.full((S, T), -1, np.int32), np.zeros(S, np.int64), np.zeros(S, np.int64)
    status = np.zeros(S, np.int32)
    q = np.arange(K ** T, dtype=np.int64)
    digit = [q // K ** t % K for t in range(T)]                           # k_t of every q
    for s in range(S):
        el = [[True if eligible is None else int(eligible[s][t * K + k]) != 0 for k in range(K)] for t in range(T)]
        un = [0] * R if unary is None else [int(x) for x in unary[s]]
        kept = [t for t in range(T) if any(el[t])]
        rows = [t * K + k for t in kept for k in range(K) if el[t][k]]
        read = [un[r] for r in rows] + [int(W[s, r, c]) for r in rows for c in rows if r // K < c // K]
        if not kept or any(abs(v) > SCORE_MAX for v in read):
            status[s] = CH_BAD_SCORE if kept else CH_EMPTY
            continue
        status[s] = CH_OK if len(kept) == T else CH_PARTIAL
        admissible = np.ones(len(q), bool)
        for t in range(T):
            admissible &= np.array(el[t])[digit[t]] if t in kept else digit[t] == 0
        objective = np.zeros(len(q), np.int64)
        una = np.array(un, np.int64)
        for i, t in enumerate(kept):
            objective += una[t * K + digit[t]]
            for u in kept[i + 1:]:
                objective += W[s][t * K + digit[t], u * K + digit[u]]
        which = np.nonzero(admissible)[0]
        values = objective[which]
        best[s], first[s] = values.max(), values[0]
        at = int(which[int(np.argmax(values))])                           # argmax: the first of equal values - the smallest q
        for t in kept:
            choice[s, t] = at // K ** t % K
    return dict(choice=choice, best=best, first=first, status=status)
