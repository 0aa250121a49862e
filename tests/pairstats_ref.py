"""Numpy restatement of the pair-statistics kernel (csrc/pairstats.hip, include/musehip_stats.h: which pairs count, what is summed
and counted) and of evaluation.GenerationTotals, the model the device code is compared with.  The similarity itself, its float64 judge
and its error bound are tests/evaluate_ref.py's (sim32 / sim64 / bound): the kernel calls the device function the nearest-neighbour
kernel calls.

Accumulation bound: a sum of c float64 terms added one by one in ANY order is within gamma(c) * sum |terms| of the exact sum, with
gamma(c) = (c - 1) u / (1 - (c - 1) u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); an fp32
similarity converts to float64 exactly, so that is the whole error of sum[i] against the exact sum of the kernel's own similarities."""
import math

import numpy as np

import evaluate_ref as ev

U = 2.0 ** -53
DEFAULT_THRESHOLD = 1 - 2.0 ** -16


def gamma(c):
    """the recursive-summation constant for c terms (0 for at most one term: nothing is rounded)"""
    c = np.maximum(np.asarray(c, np.float64) - 1, 0)
    return c * U / (1 - c * U)


def counted(nq, nk, q_valid=None, k_valid=None, q_group=None, k_group=None, self_mode=False):
    """bool [nq, nk]: pair (i, j) counts iff query row i and key row j are valid, their group ids are equal (None: id 0 on that side)
    and, in self mode, j != i"""
    qv = np.ones(nq, bool) if q_valid is None else np.asarray(q_valid) != 0
    kv = np.ones(nk, bool) if k_valid is None else np.asarray(k_valid) != 0
    qg = np.zeros(nq, np.int64) if q_group is None else np.asarray(q_group, np.int64)
    kg = np.zeros(nk, np.int64) if k_group is None else np.asarray(k_group, np.int64)
    on = qv[:, None] & kv[None, :] & (qg[:, None] == kg[None, :])
    if self_mode:
        assert nq == nk
        on &= ~np.eye(nq, dtype=bool)
    return on


def reduce_rows(sim, on, threshold=None):
    """the four outputs from an fp32 similarity matrix and the counted-pair mask: sum (float64, each row's exact sum correctly rounded:
    math.fsum), count, nan, above (None without a threshold; the comparison is fp32's, a NaN threshold counts nothing)"""
    sim = np.asarray(sim, np.float32)
    isnan = np.isnan(sim)
    fin = on & ~isnan
    total = np.array([math.fsum(sim[i, fin[i]].astype(np.float64).tolist()) for i in range(len(sim))], np.float64)
    above = None
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            above = (fin & (sim >= np.float32(threshold))).sum(1).astype(np.int32)
    return total, fin.sum(1).astype(np.int32), (on & isnan).sum(1).astype(np.int32), above


def abs_rows(sim, on):
    """sum_j |s_ij| over the counted non-NaN pairs of each row, float64"""
    s = np.where(on & ~np.isnan(sim), np.abs(np.asarray(sim, np.float64)), 0.0)
    return s.sum(1)


def pair_stats(q, k=None, q_valid=None, k_valid=None, q_group=None, k_group=None, threshold=None, sim=None):
    """the kernel's answer (sum, count, nan, above) from numpy rows; k=None: the self mode, q_valid and q_group serve both sides.
    sim: the fp32 matrix to reduce (default: evaluate_ref.sim32 of the rows)"""
    self_mode = k is None
    kk = q if self_mode else k
    if self_mode:
        k_valid, k_group = q_valid, q_group
    if sim is None:
        sim = ev.sim32(q, kk)
    return reduce_rows(sim, counted(len(q), len(kk), q_valid, k_valid, q_group, k_group, self_mode), threshold)


def best_of(sim, q_valid=None, k_valid=None):
    """metric.nearest(..., return_values=True) on a two-set matrix -> (most, best): evaluate_ref.select"""
    return ev.select(np.asarray(sim, np.float32), q_valid, k_valid)


def evaluate_generated(sample, mask, strict=False):
    """evaluation.evaluate_generated on numpy rows -> dict(valid [B], valid_count, vec [B, 56] (rows that did not decode: zeros),
    counts (CP total, CP wrong, CV total, CV wrong) over the valid rows, fatal)"""
    import decode_ref as dr
    from oracle import batch as ob
    B, L = sample.shape
    dec = [dr.decode_row(sample[b], mask[b], min(2 * L, dr.MAX_ROW), L, L, strict) for b in range(B)]
    status = np.array([d["status"] for d in dec])
    valid = status == dr.OK
    fatal = max([int(s) for s in status if s != dr.OK and s not in ev.INVALID] + [0])
    vec = np.zeros((B, 56), np.float32)
    for b in np.flatnonzero(valid):
        vec[b] = ob.msim_vectors(list(dec[b]["restored"]) + [0], ref_unbound=False)
    rows = np.flatnonzero(valid)
    (tp, wp), (tv, wv) = ob.controllability([dec[b]["meta"] for b in rows], [dec[b]["restored"] for b in rows])
    return dict(valid=valid, valid_count=int(valid.sum()), vec=vec, counts=(tp, wp, tv, wv), fatal=fatal)


class GenTotals:
    """evaluation.GenerationTotals in numpy.  update(vec [B, 56], valid [B], counts (CP total, CP wrong, CV total, CV wrong), groups);
    summary(sim=None, corpus_sim=None): the matrices to reduce (default: sim32 of the kept rows / of the rows against the corpus)"""

    def __init__(self, duplicate_threshold=DEFAULT_THRESHOLD, corpus=None, corpus_valid=None):
        self.threshold, self.corpus, self.corpus_valid = duplicate_threshold, corpus, corpus_valid
        self.vec, self.valid, self.groups, self.counts = [], [], [], np.zeros(4, np.int64)

    def update(self, vec, valid, counts, groups=None):
        self.vec.append(np.asarray(vec, np.float32))
        self.valid.append(np.asarray(valid) != 0)
        self.groups.append(np.zeros(len(vec), np.int32) if groups is None else np.asarray(groups, np.int32))
        self.counts += np.asarray(counts, np.int64)
        return self

    def summary(self, sim=None, corpus_sim=None):
        """-> (the dict, tol): tol[key] bounds |ratio - this restatement's| for a device that sums the same fp32 similarities in float64
        in any order (both sums within gamma(N) sum |s| of the exact one; the division and the subtraction round once each)"""
        div = lambda a, b: float(a) / float(b) if b else float("nan")
        vec, valid, groups = np.concatenate(self.vec), np.concatenate(self.valid), np.concatenate(self.groups)
        if sim is None:
            sim = ev.sim32(vec, vec)
        on = counted(len(vec), len(vec), valid, valid, groups, groups, True)
        total, count, nan, above = reduce_rows(sim, on, self.threshold)
        n_valid, pairs = int(valid.sum()), int(count.sum())
        out = {"valid": n_valid, "pairs": pairs // 2, "nan_pairs": int(nan.sum()) // 2, "diversity": 1 - div(math.fsum(total.tolist()), pairs),
               "duplicates": div(int((valid & (above > 0)).sum()), n_valid), "cp": div(self.counts[1], self.counts[0]),
               "cv": div(self.counts[3], self.counts[2])}
        tol = {"diversity": (2 * float(gamma(pairs)) * float(abs_rows(sim, on).sum()) / pairs + 4 * U) if pairs else 0.0}
        if self.corpus is not None:
            if corpus_sim is None:
                corpus_sim = ev.sim32(vec, self.corpus)
            most, best = best_of(corpus_sim, valid, self.corpus_valid)
            found = valid & (most >= 0) & ~np.isnan(best)
            with np.errstate(invalid="ignore"):
                hit = found & (best >= np.float32(self.threshold))
            out["novelty"] = 1 - div(math.fsum(best[found].astype(np.float64).tolist()), int(found.sum()))
            out["memorised"] = div(int(hit.sum()), n_valid)
            nf = int(found.sum())
            tol["novelty"] = (2 * float(gamma(nf)) * float(np.abs(best[found].astype(np.float64)).sum()) / nf + 4 * U) if nf else 0.0
        return out, tol
