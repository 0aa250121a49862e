"""GPU: mhs_msim_pair_stats through the C ABI (include/musehip_stats.h) at the sizes where its handling of a key changes hands - the
tile of mhs_pair_key_tile() rows, the wave's quarter and the slice's sixteenth of it, the 64 query rows of a block - with every output
sentinel-filled between guard bands and every element judged, under masks, group ids, NaN rows, planted duplicates and thresholds.

How an output is judged (tests/pairstats_ref.py, tests/evaluate_ref.py):
  * count, nan, above EQUAL the rules applied to the fp32 matrix metric.nearest(..., return_sim=True) returns for the same rows: one
    device function computes a pair's similarity for both kernels, so the bits are the same;
  * independently, #(s64 >= thr + b) <= above[i] <= #(s64 >= thr - b) over the counted pairs, s64 the float64 similarity and b
    evaluate_ref.bound (tau = 58 * 2^-24 times the product of the absolute dots);
  * sum[i] is within gamma(c) sum |s_j| of the exactly rounded sum of that fp32 matrix's counted entries, c = count[i],
    gamma(c) = (c - 1) 2^-53 / (1 - (c - 1) 2^-53): recursive float64 summation in any order;
  * and within sum_j b(i, j) + gamma(c) sum |s_j| of the sum of the float64 similarities."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate_ref as ev  # noqa: E402
import pairstats_ref as pr  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402

DEV = "cuda"
GUARD = 64
SUM_FILL, COUNT_FILL, NAN_FILL, ABOVE_FILL = -12345.5, -777, -888, -999
DEFAULT = pr.DEFAULT_THRESHOLD


def T():
    return int(_lib.lib().mhs_pair_key_tile())


def size(name):
    t = T()
    return {"T-1": t - 1, "T": t, "T+1": t + 1, "2T+1": 2 * t + 1}.get(name) or int(name)


SIZES = ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "2T+1", "257"]


def guarded(n, dtype, fill):
    return torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dtype)


def dev_i32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def call(q, k=None, q_valid=None, k_valid=None, q_group=None, k_group=None, threshold=DEFAULT, want_above=True):
    """mhs_msim_pair_stats through the C ABI on numpy inputs (k=None: self mode, q_valid and q_group serve both sides) ->
    (sum, count, nan, above) numpy; the outputs start sentinel-filled and the guard bands on both sides of each must come back untouched"""
    self_mode = k is None
    dq = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    dk = dq if self_mode else torch.from_numpy(np.ascontiguousarray(k, np.float32)).to(DEV)
    nq, nk = dq.shape[0], dk.shape[0]
    dqv, dqg = dev_i32(q_valid), dev_i32(q_group)
    dkv, dkg = (dqv, dqg) if self_mode else (dev_i32(k_valid), dev_i32(k_group))
    total = guarded(nq, torch.float64, SUM_FILL)
    count, nan, above = (guarded(nq, torch.int32, f) for f in (COUNT_FILL, NAN_FILL, ABOVE_FILL))
    got = _lib.lib().mhs_msim_pair_stats(dq.data_ptr(), nq, dk.data_ptr(), nk, _lib.ptr(dqv), _lib.ptr(dkv), _lib.ptr(dqg), _lib.ptr(dkg),
                                         int(self_mode), float(threshold), total.data_ptr() + 8 * GUARD, count.data_ptr() + 4 * GUARD,
                                         nan.data_ptr() + 4 * GUARD, above.data_ptr() + 4 * GUARD if want_above else None, _lib.current_stream())
    assert got == 0, _lib.lib().mh_last_error()
    torch.cuda.synchronize()
    for buf, fill in ((total, SUM_FILL), (count, COUNT_FILL), (nan, NAN_FILL), (above, ABOVE_FILL)):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all(), "guard band written"
    if not want_above:
        assert (above == ABOVE_FILL).all(), "above = NULL, and something was written"
    return tuple(b[GUARD:-GUARD].cpu().numpy() for b in (total, count, nan, above))


def device_matrix(q, k, q_valid, k_valid):
    """the fp32 similarity matrix of the nearest-neighbour kernel for the same rows (two-set call: the diagonal is not replaced);
    NaN where a masked row or column was skipped - those pairs are not counted either"""
    dq = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    dk = torch.from_numpy(np.ascontiguousarray(k, np.float32)).to(DEV)
    valid = None if q_valid is None else dev_i32(q_valid)
    keys_valid = None if k_valid is None else dev_i32(k_valid)
    return metric.nearest(dq, dk, valid=valid, keys_valid=keys_valid, return_sim=True)[1].cpu().numpy()


def judge(got, q, k=None, q_valid=None, k_valid=None, q_group=None, k_group=None, threshold=DEFAULT, sim=None):
    """every element of sum / count / nan / above of one call -> (sim fp32 of the device, the counted-pair mask)"""
    total, count, nan, above = got
    self_mode = k is None
    kk = q if self_mode else k
    if self_mode:
        k_valid, k_group = q_valid, q_group
    if sim is None:
        sim = device_matrix(q, kk, q_valid, k_valid)
    on = pr.counted(len(q), len(kk), q_valid, k_valid, q_group, k_group, self_mode)
    want_total, want_count, want_nan, want_above = pr.reduce_rows(sim, on, threshold)
    assert np.array_equal(count, want_count), np.flatnonzero(count != want_count)[:8]
    assert np.array_equal(nan, want_nan), np.flatnonzero(nan != want_nan)[:8]
    assert np.array_equal(above, want_above), np.flatnonzero(above != want_above)[:8]
    off = ~on.any(1)
    assert (total[off] == 0).all() and not np.signbit(total[off]).any() and (count[off] == 0).all() and (nan[off] == 0).all() and (above[off] == 0).all()
    # above between the float64 counts at thr + b and thr - b
    s64, bd = ev.sim64(q, kk), ev.bound(q, kk)
    fin = on & ~np.isnan(s64)
    assert np.array_equal(on & np.isnan(sim), on & np.isnan(s64))
    thr = float(np.float32(threshold))
    with np.errstate(invalid="ignore"):
        lo, hi = (fin & (s64 >= thr + bd)).sum(1), (fin & (s64 >= thr - bd)).sum(1)
    assert (lo <= above).all() and (above <= hi).all(), np.flatnonzero((lo > above) | (above > hi))[:8]
    # sum against the device's own fp32 values, and against float64
    g = pr.gamma(count) * pr.abs_rows(sim, on)
    assert (np.abs(total - want_total) <= g).all(), float((np.abs(total - want_total) - g).max())
    assert (total[count <= 1] == want_total[count <= 1]).all()                          # nothing to round
    t64 = np.where(fin, s64, 0.0).sum(1)
    b64 = np.where(fin, bd, 0.0).sum(1)
    own = pr.gamma(on.shape[1]) * np.where(fin, np.abs(s64), 0.0).sum(1)                 # numpy's own summation of the float64 row
    assert (np.abs(total - t64) <= b64 + g + own).all(), float((np.abs(total - t64) - b64 - g).max())
    if self_mode:                                                                        # the implied pair relation is symmetric
        assert above.sum() % 2 == 0 and count.sum() % 2 == 0 and nan.sum() % 2 == 0
        upper = on & np.triu(np.ones_like(on), 1) & ~np.isnan(sim)
        twice = 2 * math.fsum(sim[upper].astype(np.float64).tolist())
        assert abs(math.fsum(total.tolist()) - twice) <= float(g.sum()) + 4 * pr.U * abs(twice)
    return sim, on


def check(q, k=None, q_valid=None, k_valid=None, q_group=None, k_group=None, threshold=DEFAULT, sim=None):
    got = call(q, k, q_valid, k_valid, q_group, k_group, threshold)
    sim, on = judge(got, q, k, q_valid, k_valid, q_group, k_group, threshold, sim)
    return got + (sim, on)


def vectors(n, seed):
    return ev.unit_vectors(np.random.default_rng(seed), n)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("name", SIZES)
def test_self_mode_sizes(name):
    n = size(name)
    v = vectors(n, 300 + n)
    if n > 2:
        v[n - 1] = v[0]                                                                  # a duplicate from the first row to the last
    total, count, nan, above, sim, _ = check(v)
    assert (count == n - 1).all() and (nan == 0).all()
    if n == 1:
        assert total.tolist() == [0.0] and above.tolist() == [0]                        # a row is no pair with itself
    if n > 2:
        assert above[0] == 1 and above[n - 1] == 1 and above.sum() == 2
    assert same_bits(call(v), call(v)), "the same call, other bits"
    none = call(v, want_above=False)                                                     # above = NULL: the rest is the same
    assert same_bits(none[:3], (total, count, nan))
    check(v, threshold=0.0, sim=sim)


@pytest.mark.parametrize("nq,nk", [("1", "257"), ("65", "3"), ("257", "1"), ("T+1", "2T+1")])
def test_two_set_mode_sizes(nq, nk):
    nq, nk = size(nq), size(nk)
    q, k = vectors(nq, 7 * nq + nk), vectors(nk, 11 * nk + nq)
    k[nk - 1] = q[0]
    total, count, nan, above, _, _ = check(q, k)
    assert (count == nk).all() and above[0] == 1 and above.sum() == 1                    # the diagonal is a pair like any other here
    if nq > 3:                                                                           # another grid for the same pairs
        part = call(q[3:], k)
        assert same_bits(part, (total[3:], count[3:], nan[3:], above[3:]))


def test_dataset_scale_and_another_geometry():
    """4096 x 4096 in self mode, every element judged; then the same rows launched with another number of slices per wave (the query
    set decides: one slice from 64 x CUs rows on, four for a small set): equal integers, sums within 2 gamma sum |s|"""
    v = vectors(4096, 11)
    v[[77, 4000]] = v[5]
    total, count, nan, above, sim, on = check(v)
    assert (count == 4095).all() and above[[5, 77, 4000]].tolist() == [2, 2, 2] and above.sum() == 6
    keys = v[:300]
    big = np.tile(v, (5, 1))[:64 * 256 + 70]
    t_big, c_big, n_big, a_big = call(big, keys, threshold=0.0)
    few = slice(3000, 3100)
    got_few = call(big[few], keys, threshold=0.0)
    judge(got_few, big[few], keys, threshold=0.0)
    t_few, c_few, n_few, a_few = got_few
    assert np.array_equal(c_big[few], c_few) and np.array_equal(n_big[few], n_few) and np.array_equal(a_big[few], a_few)
    g = 2 * pr.gamma(c_few) * np.abs(sim[few, :300].astype(np.float64)).sum(1)            # rows 3000.. of big are rows 3000.. of v
    assert (np.abs(t_big[few] - t_few) <= g).all()
    assert same_bits((t_big[:4096], c_big[:4096], a_big[:4096]), (t_big[4096:8192], c_big[4096:8192], a_big[4096:8192]))


# ------------------------------------------------------------------------------------------------ planted inputs
def test_duplicated_rows_on_both_sides_of_every_seam():
    """identical pieces reach the default threshold wherever the two copies are handled: across a tile seam, a wave's quarter-tile seam, a
    slice's sixteenth-tile seam, and between two tiles' different quarters"""
    t = T()
    q = vectors(70, 1)
    seams = ((t - 1, t), (t // 4 - 1, t // 4), (t // 16 - 1, t // 16), (t // 2 + 3, t + t // 4 + 5), (0, 2 * t), (t - 1, 2 * t))
    for a, b in seams:
        k = vectors(2 * t + 1, 2)
        k[a] = k[b] = q[a % 70]
        _, _, _, above, sim, _ = check(q, k)
        assert above[a % 70] == 2 and above.sum() == 2 and np.array_equal(sim[:, a].view(np.int32), sim[:, b].view(np.int32)), (a, b)
    for a, b in seams:                                                                   # self mode: each copy finds the other, not itself
        v = vectors(2 * t + 1, 3)
        v[b] = v[a]
        _, _, _, above, _, _ = check(v)
        assert above[a] == 1 and above[b] == 1 and above.sum() == 2, (a, b)


def test_rows_orthogonal_to_everything():
    """a zero harmony part makes every similarity of the row exactly 0: it is counted, adds nothing, and reaches the threshold 0 only"""
    n = T() + 9
    v = vectors(n, 4)
    z = v.copy()
    z[:, 44:] = 0
    total, count, _, above, sim, _ = check(z, threshold=0.0)
    assert (total == 0).all() and (count == n - 1).all() and (above == n - 1).all()
    assert (check(z, threshold=float(np.float32(1e-30)), sim=sim)[3] == 0).all()
    v[[0, 5, 64, T()], 44:] = 0
    total, count, _, _, _, _ = check(v)
    assert (total[[0, 5, 64, T()]] == 0).all() and (count == n - 1).all()
    total, _, _, above, _, _ = check(v[:7], z, threshold=0.0)
    assert (total == 0).all() and (above == n).all()


def test_nan_rows_as_keys_and_as_queries():
    t = T()
    k = vectors(2 * t + 1, 5)
    k[[t + 2, 7, 2 * t], 44:] = np.nan       # the reference's 0 / 0 harmony vector of a row without notes
    q = vectors(66, 6)
    _, count, nan, _, _, _ = check(q, k)
    assert (nan == 3).all() and (count == 2 * t - 2).all()
    kv = np.ones(2 * t + 1, np.int32)
    kv[7] = 0
    assert (check(q, k, k_valid=kv)[2] == 2).all()
    q[[0, 65]] = np.nan
    total, count, nan, above, _, _ = check(q, vectors(t + 1, 7), threshold=0.0)
    assert count[[0, 65]].tolist() == [0, 0] and nan[[0, 65]].tolist() == [t + 1] * 2 and total[[0, 65]].tolist() == [0, 0] and above[[0, 65]].tolist() == [0, 0]
    v = vectors(t + 1, 8)
    v[[0, 70], 44:] = np.nan                 # self mode: a NaN row's own diagonal is not counted as a NaN pair
    _, count, nan, _, _, _ = check(v)
    assert nan[[0, 70]].tolist() == [t, t] and count[[0, 70]].tolist() == [0, 0] and (np.delete(nan, [0, 70]) == 2).all()


# ------------------------------------------------------------------------------------------------ masks and groups
def masks(n, t):
    one = np.zeros(n, np.int32)
    one[t] = 1
    tile = np.ones(n, np.int32)
    tile[t:2 * t] = 0
    return {"none": None, "nothing valid": np.zeros(n, np.int32), "one row": one, "alternating": (np.arange(n) % 2).astype(np.int32),
            "a whole tile": tile, "nonzero values": ((np.arange(n) % 3) * -5).astype(np.int32)}


def groups(n, t):
    return {"none": None, "all distinct": np.arange(n, dtype=np.int32) - 3, "two interleaved": (np.arange(n) % 2).astype(np.int32),
            "one per tile": (np.arange(n) // t).astype(np.int32),
            "negative and extreme ids": np.where(np.arange(n) % 3 == 0, -2 ** 31, np.where(np.arange(n) % 3 == 1, -1, 2 ** 31 - 1)).astype(np.int32)}


@pytest.mark.parametrize("mask", ["none", "nothing valid", "one row", "alternating", "a whole tile", "nonzero values"])
def test_validity_masks(mask):
    t = T()
    n = 2 * t + 1
    v, q = vectors(n, 9), vectors(67, 10)
    m = masks(n, t)[mask]
    sim_self = device_matrix(v, v, None, None)
    total, count, nan, above, _, on = check(v, q_valid=m, threshold=0.0, sim=sim_self)
    valid = np.ones(n, bool) if m is None else m != 0
    assert np.array_equal(count, np.where(valid, valid.sum() - 1, 0))
    if mask == "one row":
        assert not on.any() and (total == 0).all()                                       # its own diagonal is its only partner: no pair
    sim_two = device_matrix(q, v, None, None)
    _, count, _, _, _, _ = check(q, v, k_valid=m, threshold=0.0, sim=sim_two)
    assert (count == valid.sum()).all()
    check(q, v, q_valid=(np.arange(67) % 3 > 0).astype(np.int32), k_valid=m, sim=sim_two)


@pytest.mark.parametrize("group", ["none", "all distinct", "two interleaved", "one per tile", "negative and extreme ids"])
def test_group_ids_alone_and_with_masks(group):
    t = T()
    n = 2 * t + 1
    v, q = vectors(n, 12), vectors(67, 13)
    dup = (t - 1, t, t + 1)
    v[t] = v[t + 1] = v[t - 1]                                                           # three copies of one row across the tile seam
    g = groups(n, t)[group]
    sim_self, sim_two = device_matrix(v, v, None, None), device_matrix(q, v, None, None)
    _, count, _, above, _, _ = check(v, q_group=g, sim=sim_self)
    gid = np.zeros(n, np.int64) if g is None else g.astype(np.int64)
    assert np.array_equal(count, np.array([(gid == x).sum() - 1 for x in gid]))
    if group == "all distinct":
        assert (count == 0).all()
    assert above.sum() == sum(gid[x] == gid[y] for x in dup for y in dup if x != y)      # copies count only inside one group
    qg = None if g is None else g[:67][::-1].copy()
    _, count, _, _, _, _ = check(q, v, q_group=qg, k_group=g, threshold=0.0, sim=sim_two)
    if g is not None:                                                                    # a NULL side is group 0
        _, c0, _, _, _, _ = check(q, v, q_group=None, k_group=g, threshold=0.0, sim=sim_two)
        assert (c0 == (gid == 0).sum()).all()
        check(q, v, q_group=qg, k_group=None, sim=sim_two)
    for mask in ("alternating", "a whole tile", "one row"):                              # masks and groups combined
        m = masks(n, t)[mask]
        check(v, q_valid=m, q_group=g, threshold=0.0, sim=sim_self)
        check(q, v, q_valid=(np.arange(67) % 3 > 0).astype(np.int32), k_valid=m, q_group=qg, k_group=g, sim=sim_two)


# ------------------------------------------------------------------------------------------------ thresholds
def test_thresholds():
    t = T()
    v = vectors(2 * t + 1, 14)
    _, _, _, _, sim, on = check(v)
    i = t + 3
    row = np.where(on[i], sim[i], -1)
    j = int(np.argsort(row)[-5])                                                         # the fifth largest of a row, read from the kernel's matrix
    value = float(sim[i, j])
    assert value > 0 and (row == sim[i, j]).sum() == 1
    above = check(v, threshold=value, sim=sim)[3]
    assert above[i] == 5 and above[j] >= 1                                               # >=: the pair itself counts (with > it would be 4)
    nxt = float(np.nextafter(np.float32(value), np.float32(2)))
    assert check(v, threshold=nxt, sim=sim)[3][i] == 4
    _, count, _, above, _, _ = check(v, threshold=0.0, sim=sim)
    assert np.array_equal(above, count)                                                  # no similarity of non-negative rows is below 0
    assert (check(v, threshold=2.0, sim=sim)[3] == 0).all()                              # above every similarity
    assert (check(v, threshold=float("nan"), sim=sim)[3] == 0).all()
    assert (check(v, threshold=float("-inf"), sim=sim)[3] == count).all()
    # the default threshold is exact in fp32 and the device sees that value
    assert check(v, threshold=np.float64(DEFAULT), sim=sim)[3].sum() == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_call_they_guard():
    L = _lib.lib()
    a, b = torch.zeros(4, 56, device=DEV), torch.zeros(4, 56, device=DEV)
    ints = torch.ones(4, 4, device=DEV, dtype=torch.int32)
    total = torch.zeros(4, device=DEV, dtype=torch.float64)
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def run(q, nq, k, nk, qv, kv, qg, kg, self_mode, total=total, count=ints[1], nan=ints[2]):
        return L.mhs_msim_pair_stats(P(q), nq, P(k), nk, P(qv), P(kv), P(qg), P(kg), self_mode, 0.5, P(total), P(count), P(nan), P(ints[3]),
                                     _lib.current_stream())
    for args in ((a, 4, b, 4, None, None, None, None), (a, 4, a, 3, None, None, None, None), (a, 4, a, 4, ints[0], None, None, None),
                 (a, 4, a, 4, None, None, ints[0], None), (a, 4, a, 4, None, None, None, ints[0])):
        assert run(*args, 1) == _lib.MH_ERR_INVALID and b"self = 1" in L.mh_last_error()
    assert run(a, 4, a, 4, None, None, None, None, 2) == _lib.MH_ERR_INVALID and b"neither 0 nor 1" in L.mh_last_error()
    assert run(a, 0, a, 4, None, None, None, None, 0) == _lib.MH_ERR_INVALID and b"outside" in L.mh_last_error()
    for kw in (dict(total=None), dict(count=None), dict(nan=None)):
        assert run(a, 4, b, 4, None, None, None, None, 0, **kw) == _lib.MH_ERR_INVALID and b"NULL" in L.mh_last_error()
    assert (ints == 1).all() and (total == 0).all(), "a refused call wrote something"
    assert run(a, 4, a, 4, ints[0], ints[0], ints[0], ints[0], 1) == 0
    torch.cuda.synchronize()
    assert ints[1].tolist() == [3] * 4 and ints[2].tolist() == [0] * 4 and ints[3].tolist() == [0] * 4 and total.tolist() == [0.0] * 4
