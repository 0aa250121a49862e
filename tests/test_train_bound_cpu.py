"""The training parity matrix's bounds hold for plain float32 arithmetic (CPU): each reduction kernel of csrc/train.hip restated in float32
numpy (tests/train_ref.py: *_emulate - the kernel's formula order, numpy's summation order) stays within HALF of the per-element bound of
its float64 reference, at the matrix' own inputs: the case lists of tests/test_train_matrix_gpu.py, drawn by the same functions and seeds
(tests/train_ref.py: *_inputs).  A bound this emulation could not meet with
that margin would be wrong; what it does not contain - the kernels' summation order, FMA contraction, the device's tanhf / erff / expf /
logf - is what the matrix measures on the GPU.  Where the output is stored as bf16, the float32 result BEFORE that rounding is held to half
the bound and the stored one to the whole of it (`within`): bf16 keeps 8 significant bits, so rounding to nearest alone costs up to 2^-8
relative - all of the bound's output term, of which no margin can be asked.  The ulp allowance of those four functions (train_ref.MATH_ULP) is checked the same way
against numpy's float32 functions (torch's float32 erf: numpy has none)."""
import numpy as np
import pytest

import test_train_matrix_gpu as tm
import train_ref as tr

HALF = 0.5


def _check(what, got, pair, worst):
    r = tr.ratio(got, *pair)
    print("TRAIN-BOUND %s %.3f" % (what, r))
    worst[what] = r


def within(got, pair, dtype=tr.F32):
    """the float32 result within half the bound; once stored in `dtype`, within the bound"""
    return tr.ratio(got, *pair) <= HALF and tr.ratio(tr.q(got, dtype), *pair) <= 1.0


@pytest.mark.parametrize("case", tm.LN_CASES, ids=tm._ln_id)
def test_layernorm_backward_emulation_within_half_the_bound(case):
    H, rows, P, dtype, adj, acc, eps, entry, p, always, panel = case
    x, dy, gamma, start_g, start_b = tr.ln_case_inputs(H, rows, P, acc, dtype)
    ref = tr.ln_bwd(x, dy, gamma, eps, dtype, start_g, start_b)
    dx, dg, db = tr.ln_bwd_emulate(x, dy, gamma, eps, dtype)
    if acc:
        dg, db = start_g + dg, start_b + db
    worst = {}
    _check("dx", dx, ref["dx"], worst)
    _check("dgamma", dg, ref["dgamma"], worst)
    _check("dbeta", db, ref["dbeta"], worst)
    assert all(w <= HALF for w in worst.values()), worst
    assert tr.ratio(tr.q(dx, dtype), *ref["dx"]) <= 1.0
    if entry != "plain" and (p > 0 or always):
        # the second output, made of the emulation's OWN rounded dx (the rounding may differ from the reference's by a whole ulp)
        keep = tr.rng(H).uniform(size=dx.shape) >= p
        rs = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        got = tr.q(np.where(keep, tr.q(dx, dtype) * rs, np.float32(0)), dtype)
        m_ref = tr.ln_dropped(ref["dx"][0], ref["dx_arith"], keep, p, dtype)
        assert tr.ratio(got, *m_ref) <= 1.0 and np.all(m_ref[0][~keep] == 0) and np.all(m_ref[1][~keep] == 0)
    if rows > 1:
        # the bound is no multiple of max |dx|: it sees s1 standing in for s2 in the dx line
        f = np.float32
        xx, dd, gg = x.astype(f), dy.astype(f), gamma.astype(f)
        mean = xx.mean(1, keepdims=True)
        rstd = 1 / np.sqrt(((xx - mean) ** 2).mean(1, keepdims=True) + f(eps))
        s1 = (dd * gg).mean(1, keepdims=True)
        wrong = rstd * (dd * gg - s1 - (xx - mean) * rstd * s1)
        assert tr.ratio(tr.q(wrong, dtype), *ref["dx"]) > 1.0


def test_dropped_copy_bound_covers_a_whole_ulp_flip():
    """dx stored one bf16 ulp away from the reference's rounding, everywhere and in either direction (the most a flipped rounding costs),
    stays within the dropped copy's bound once dx's own arithmetic bound is added"""
    H, rows, P, dtype = 128, 263, 64, tr.BF16
    x, dy, gamma, _, _ = tr.ln_case_inputs(H, rows, P, 0, dtype)
    ref = tr.ln_bwd(x, dy, gamma, 1e-5, dtype)
    stored = tr.q(ref["dx"][0], dtype)
    keep = tr.rng(1).uniform(size=stored.shape) >= 0.1
    m_ref = tr.ln_dropped(ref["dx"][0], ref["dx_arith"], keep, 0.1, dtype)
    rs = np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    for step in (1, -1):
        flipped = (stored.view(np.int32) + step * 0x10000).view(np.float32)
        got = tr.q(np.where(keep, flipped * rs, np.float32(0)), dtype)
        # (a flip happens only where the exact dx sits within its arithmetic bound of a rounding boundary: the bound is checked without
        # that term, which is the stricter statement)
        err = np.abs(got.astype(np.float64) - m_ref[0])
        assert np.all(err <= m_ref[1] - np.where(keep, ref["dx_arith"] * float(rs), 0.0) + 1e-300)


@pytest.mark.parametrize("case", tm.COLSUM_CASES, ids=tm._colsum_id)
def test_column_sum_emulation_within_half_the_bound(case):
    cols, ld, rows, P, batch, acc, dtype, off = case
    _, _, x, start = tr.colsum_inputs(cols, ld, rows, P, batch, acc, dtype)
    got = x.sum(1, dtype=np.float32)
    if acc:
        got = start + got
    assert tr.ratio(got, *tr.col_sum(x, start)) <= HALF
    if rows >= 64:     # ... and sees one row missing (a dropped term of the unrolled fold)
        assert tr.ratio(got - x[:, -1, :], *tr.col_sum(x, start)) > 1.0


@pytest.mark.parametrize("n,E,V,clamp", tm.SCATTER_CASES[:-1])      # (the last is the wrap shape: 5 tokens, nothing a sum could lose)
def test_scatter_add_emulation_within_half_the_bound(n, E, V, clamp):
    src, ids, table = tr.scatter_inputs(n, E, V, clamp)
    got = table.copy()
    cl = np.clip(ids, 0, V - 1)
    for v in np.unique(cl):
        got[v] += src[cl == v].sum(0, dtype=np.float32)
    assert tr.ratio(got, *tr.scatter_add_rows(src, ids, table, V)) <= HALF


@pytest.mark.parametrize("V,n,odd", tm.CE_CASES)
def test_cross_entropy_emulation_within_half_the_bound(V, n, odd):
    logits, target, gs = tr.ce_inputs(n, V)
    ref = tr.ce_fwd(logits, target, V)
    lse, loss = tr.ce_fwd_emulate(logits, target, V)
    assert tr.ratio(lse, *ref["lse"]) <= HALF and tr.ratio(loss, *ref["loss"]) <= HALF
    lse32 = ref["lse"][0].astype(np.float32)
    for dtype in (tr.BF16, tr.F32):
        oh = np.zeros((n, V), np.float32)
        oh[np.arange(n), np.clip(target, 0, V - 1)] = 1
        got = (np.exp(logits - lse32[:, None]) - oh) * gs[:, None]
        assert within(got, tr.ce_bwd(logits, target, lse32, gs, V, dtype), dtype)


@pytest.mark.parametrize("per_batch,B,with_b,scale_a,off", tm.SQDIFF_MEAN_CASES)
def test_squared_error_emulation_within_half_the_bound(per_batch, B, with_b, scale_a, off):
    a, b = tr.sqdiff_inputs(per_batch, B, with_b)
    assert tr.ratio(tr.sqdiff_mean_emulate(a, b, scale_a), *tr.sqdiff_mean(a, b, scale_a)) <= HALF


@pytest.mark.parametrize("dtype", [tr.BF16, tr.F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("L,rows,scale", tm.SOFTMAX_CASES)
def test_softmax_emulation_within_half_the_bound(L, rows, scale, dtype):
    s, dp = tr.softmax_inputs(L, rows, scale, dtype)
    ref = tr.softmax_rows(s, scale, dtype)
    assert within(tr.softmax_rows_emulate(s, scale, dtype), ref, dtype)
    p = tr.q(ref[0], dtype)
    assert within(tr.softmax_bwd_rows_emulate(p, dp, scale, dtype), tr.softmax_bwd_rows(p, dp, scale, dtype), dtype)


@pytest.mark.parametrize("act", [tr.ACT_NONE, tr.ACT_TANH, tr.ACT_GELU, tr.ACT_SILU], ids=["none", "tanh", "gelu", "silu"])
def test_float32_math_functions_within_half_the_ulp_allowance(act):
    """numpy's float32 tanh / exp (torch's float32 erf) through the kernels' formulas: within half of the bounds that give the device's
    functions MATH_ULP units in the last place"""
    x = tr.act_inputs(200003, tr.F32, seed=act)       # (a dense sweep of [-12, 12]; the matrix' own n = 1 and 255 inputs below)
    dy = tr.rng(9).standard_normal(x.shape).astype(np.float32)
    for n in (1, 255):
        for dtype in (tr.BF16, tr.F32):
            xm, dym = tr.act_inputs(n, dtype, seed=act + n), tr.q(tr.rng(n).standard_normal(n) * 2, dtype)
            assert within(tr.act_emulate(xm, act), tr.act_fwd(xm, act, dtype), dtype)
            assert within(tr.act_emulate(xm, act, dym), tr.act_bwd(dym, xm, act, dtype), dtype)
    assert tr.ratio(tr.act_emulate(x, act), *tr.act_fwd(x, act, tr.F32)) <= HALF
    assert tr.ratio(tr.act_emulate(x, act, dy), *tr.act_bwd(dy, x, act, tr.F32)) <= HALF
    xb = tr.act_inputs(4099, tr.BF16, seed=act)
    dyb = tr.q(dy[:xb.size], tr.BF16)
    assert within(tr.act_emulate(xb, act), tr.act_fwd(xb, act, tr.BF16), tr.BF16)
    assert within(tr.act_emulate(xb, act, dyb), tr.act_bwd(dyb, xb, act, tr.BF16), tr.BF16)


def test_exp_and_log_within_half_the_ulp_allowance():
    z = -tr.rng(4).uniform(0, 80, 100000).astype(np.float32)
    e = np.exp(z.astype(np.float64))
    assert np.all(np.abs(np.exp(z) - e) <= HALF * (tr.MATH_ULP * tr.U * e + tr.FLT_MIN))
    s = tr.rng(5).uniform(1, 729, 100000).astype(np.float32)
    assert np.all(np.abs(np.log(s) - np.log(s.astype(np.float64))) <= HALF * tr.MATH_ULP * tr.U * np.log(s.astype(np.float64)) + 1e-300)


def test_storage_rounding_and_layout_helpers():
    import torch
    x = tr.rng(6).standard_normal(10000).astype(np.float32) * 100
    assert np.array_equal(tr.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())
    p = tr.perm16(32)
    assert list(p[:16]) == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15] and np.array_equal(p[p], np.arange(32))
    a = np.arange(5 * 64, dtype=np.float32).reshape(5, 64)
    pan = tr.to_panel(a, 7)
    assert pan.shape == (2, 7, 32) and pan[1, 3, 4] == a[3, 36] and np.isnan(pan[:, 5:]).all() and np.array_equal(tr.from_panel(pan, 5), a)
