"""The split-precision parity matrix's bounds are neither vacuous nor too tight (CPU): each kernel of csrc/split.hip restated in float32
numpy with emulated 16-bit parts (tests/split_ref.py: *_emulate - the kernel's formula order, numpy's / BLAS' summation order; bf16 by
bit manipulation, fp16 through np.float16 with the round-toward-zero of v_cvt_pkrtz done by hand) stays within HALF of the per-element
bound of its float64 reference at the matrix' own inputs - the case lists of tests/test_split_matrix_gpu.py, drawn by the same functions
and seeds - and the same restatement with ONE injected error leaves the bound: lo parts zeroed, one of the three products dropped, the
residual's lo part skipped, bias[col] for bias[row], a rescale skipped on one key tile, alpha from the new maximum on both sides, the
unbiased variance.  What the restatement does not contain - the MFMA's summation order, the device's tanhf / erff / v_exp_f32 - is what
the matrix measures on the GPU.

Row samples: the persistent and the non-temporal-store GEMM cases are restated on the rows test_split_matrix_gpu.stream_rows names (the
first tile, the last tile, every 97th row), with the persistent cases' device-dependent M taken for a 256-CU part."""
import math

import numpy as np
import pytest

import split_ref as sr
import test_split_matrix_gpu as tm

HALF = 0.5
DT = pytest.mark.parametrize("dt", sr.DTYPES, ids=[sr.NAME[d] for d in sr.DTYPES])


def _val(x, out_mode=0):
    return x if out_mode == 2 else sr.val(x)


@DT
@pytest.mark.parametrize("case", tm.GEMM_CASES, ids=tm._gemm_id)
def test_gemm_emulation_within_half_the_bound_and_injected_errors_outside(case, dt):
    name, _, N, K, act, out_mode, bias, res, form = case
    M = tm.gemm_rows(case, 256)
    A, W, bias_v, R = tm.gemm_operands(case, M, dt)
    rows = tm.stream_rows(M) if form in tm.PERSISTENT else np.arange(M)
    sel = lambda P: tuple(p[rows] for p in P) if P is not None else None
    args = (sel(A), W, bias_v if bias == "col" else None, bias_v[rows] if bias == "row" else None, act, sel(R), out_mode, dt)
    ref = sr.gemm(*args)
    r = sr.ratio(_val(sr.gemm_emulate(*args), out_mode), *ref)
    print("SPLIT-BOUND %s %s %.3f" % (name, sr.NAME[dt], r))
    assert r <= HALF
    assert np.isfinite(ref[1]).all() and (ref[1] > 0).all()
    inject = ["lo", "hilo"] + (["reslo"] if res else []) + (["biascol"] if bias == "row" and N > 1 else [])
    for drop in inject:
        assert sr.ratio(_val(sr.gemm_emulate(*args, drop=drop), out_mode), *ref) > 1.0, drop


@DT
@pytest.mark.parametrize("K,M", tm.GEMM_LN_CASES)
def test_gemm_layernorm_emulation(K, M, dt):
    A, W, R, bias, gamma, beta = tm.gemm_ln_case(K, M, dt)
    ref = sr.gemm_ln(A, W, bias, R, gamma, beta, 1e-12, dt)
    live = np.ones(M, dtype=bool)
    if M > 3:
        live[3] = False          # (the constant row: its rstd is 1e6, the bound of every element above |y| - checked below, not injected into)
    got = sr.val(sr.gemm_ln_emulate(A, W, bias, R, gamma, beta, 1e-12, dt))
    assert sr.ratio(got, *ref) <= HALF
    if M > 3:
        assert np.array_equal(got[3], sr.val(sr.split_rn(beta, dt)))          # exactly beta: zero deviations whatever rstd is
    # (K = 2048: the worst-case accumulation term, 3 K u sum |a| |w|, is 6144 u wide - above what the bf16 lo parts carry, 2^-9 of a sum
    # that grows like sqrt(K); the injected errors are asked of the K <= 96 cases, where the matrix' own resolution lies)
    for kw in (dict(drop="lo"), dict(drop="hilo"), dict(drop="reslo"), dict(unbiased=True)) if K <= 96 else ():
        bad = sr.val(sr.gemm_ln_emulate(A, W, bias, R, gamma, beta, 1e-12, dt, **kw))
        assert sr.ratio(bad[live], ref[0][live], ref[1][live]) > 1.0, kw


@DT
@pytest.mark.parametrize("case", tm.LN_CASES, ids=tm._ln_id)
def test_layernorm_emulation(case, dt):
    H, rows, L, add, dx = case
    x, gamma, beta, pos, emb, rows_of = tm.ln_case(case)
    ref = sr.layernorm(x, pos, emb, rows_of, L, gamma, beta, 1e-12, dt)
    assert sr.ratio(sr.val(sr.layernorm_emulate(x, pos, emb, rows_of, L, gamma, beta, 1e-12, dt)), *ref) <= HALF
    # rows that are not constant: the unbiased variance leaves the bound (H = 32: 1.6 % of y; H = 2048: 2.4e-4 of y, above both part types')
    var = x.astype(np.float64).var(1) if not add else np.ones(rows)
    live = var > 1e-6
    if live.any():
        bad = sr.val(sr.layernorm_emulate(x, pos, emb, rows_of, L, gamma, beta, 1e-12, dt, unbiased=True))
        assert sr.ratio(bad[live], ref[0][live], ref[1][live]) > 1.0


@DT
@pytest.mark.parametrize("case", tm.ATTN_CASES, ids=tm._attn_id)
def test_attention_emulation(case, dt):
    dh, L, B, nh, profile, pitched, factor = case
    scale = factor / math.sqrt(dh)
    q, k, v = sr.attn_inputs(B, L, nh, dh, profile, dt, seed=dh * 1000 + L + B)
    ref = sr.attention(q, k, v, B, L, nh, dh, scale, dt)
    r = sr.ratio(sr.val(sr.attention_emulate(q, k, v, B, L, nh, dh, scale, dt)), *ref)
    print("SPLIT-BOUND %s %s %.3f" % (tm._attn_id(case), sr.NAME[dt], r))
    assert r <= HALF
    assert sr.ratio(sr.val(sr.attention_emulate(q, k, v, B, L, nh, dh, scale, dt, drop="lo")), *ref) > 1.0
    # more than one key tile: alpha = 1 on every tile where the maximum rises each time; the rescale skipped on the second tile where
    # that tile still matters to the result (plain scores: under rising ones its weights are gone by the last tile)
    for drop in {"rising": ("alpha",), "plain": ("rescale", "alpha")}.get(profile, ()) if L > 64 else ():
        assert sr.ratio(sr.val(sr.attention_emulate(q, k, v, B, L, nh, dh, scale, dt, drop=drop)), *ref) > 1.0, drop


@DT
def test_parts_and_their_error_terms(dt):
    """the emulated parts against torch's casts, and part_err / trunc_err against the emulated splits over nine decades"""
    import torch
    g = sr.rng(5)
    x = (g.standard_normal(200000) * 10.0 ** g.uniform(-7, 4, 200000)).astype(np.float32)
    T = torch.bfloat16 if dt == sr.BF16X3 else torch.float16
    assert np.array_equal(sr.rn16(x, dt), torch.from_numpy(x).to(T).float().numpy())
    v = x.astype(np.float64)
    assert np.all(np.abs(sr.val(sr.split_rn(x, dt)) - v) <= sr.part_err(v, dt))
    p = np.abs(x[np.abs(x) <= 1])
    hi, lo = sr.split_trunc(p, dt)
    assert np.all(hi <= p) and np.all(lo >= 0) and np.all(lo <= sr.trunc_lo(dt) * p + 2.0 ** -24)
    assert np.all(np.abs(sr.val((hi, lo)) - p) <= sr.trunc_err(p.astype(np.float64), dt))
    assert np.abs(sr.val((hi, lo)) - p).max() > 0.25 * sr.trunc_err(p.astype(np.float64), dt)[np.argmax(np.abs(sr.val((hi, lo)) - p))]
    # the split by rounding that the kernel does NOT use stays inside the truncation's bound too
    assert np.all(np.abs(sr.val(sr.split_rn(p, dt)) - p) <= sr.trunc_err(p.astype(np.float64), dt))
    pan = sr.to_panels((x[:320].reshape(5, 64), x[320:640].reshape(5, 64)), 7)
    assert pan.shape == (2, 2, 7, 32) and pan[1, 1, 3, 4] == x[320 + 3 * 64 + 36] and np.isnan(pan[:, :, 5:]).all()
    assert np.array_equal(sr.from_panels(pan, 5, 64)[0], x[:320].reshape(5, 64))
