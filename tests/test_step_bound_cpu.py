"""The sampling-step parity matrix's bounds hold for plain float32 arithmetic (CPU): every bounded kernel restated in float32 / bf16 numpy
(tests/step_ref.py: *_emulate) stays within HALF of the per-element bound of its float64 reference, at the matrix' own inputs - the case
lists of tests/test_step_matrix_gpu.py, drawn by the same functions and seeds.  A bound this restatement could not meet with that margin
would be wrong; what it does not contain - the kernels' summation order where numpy's stands in, FMA contraction, the device's math
functions and matrix pipe - is what the matrix measures on the GPU.  Where the output is stored as bf16, the float32 result BEFORE that
rounding is held to half the bound and the stored one to the whole of it (`within`), as in tests/test_train_bound_cpu.py.

Also here, before any GPU run: the share of rows in the near-tie class of every argbest case (at most 1 %, with the float32 restatement's
own choice passing the margin rule), the share of truncated-normal elements left out with the cap 1e-4 in place of the measured tolerance
(at most 1 % per case), and known answers of the host restatements themselves (Philox4x32-10's published test vectors, the slot fold's
tie rules, the split table)."""
import numpy as np
import pytest

import gemm_census as gc
import step_ref as sr
import test_step_matrix_gpu as sm

HALF = 0.5
F32, BF16 = sr.F32, sr.BF16


def within(got, pair, dtype=F32):
    return sr.ratio(got, *pair) <= HALF and sr.ratio(sr.q(got, dtype), *pair) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ restatements themselves
def test_philox_10_rounds_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    z = [np.zeros(1, np.uint64)] * 4
    assert [int(w[0]) for w in gc.philox7(z, 0, 0, rounds=10)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = [np.full(1, 0xffffffff, np.uint64)] * 4
    assert [int(w[0]) for w in gc.philox7(f, 0xffffffff, 0xffffffff, rounds=10)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    p = [np.full(1, v, np.uint64) for v in (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    assert [int(w[0]) for w in gc.philox7(p, 0xa4093822, 0x299f31d0, rounds=10)] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_u01_rounds_like_float32():
    r = np.array([0, 0xFF, 0x100, 0xFFFFFFFF, 0x80000100, 0x80000300], dtype=np.uint64)
    u = sr.u01(r)
    assert u.dtype == np.float32 and u[0] == np.float32(0.5 / 16777216) and u[1] == u[0] and 0 < u.min() and u.max() <= 1.0
    # above 2^23 the + 0.5 is a tie: to even
    assert u[4] == np.float32(8388609 + 0.5) * np.float32(1 / 16777216) and float(u[4]) * 16777216 == 8388610.0 and float(u[5]) * 16777216 == 8388612.0


@pytest.mark.parametrize("case", sm.TN_CASES, ids=lambda c: "bound%g-n%d" % (c[0], c[1]))
def test_truncated_normal_exclusion_share_at_the_cap(case):
    bound, n, first, seed, stream, step = case
    z, near, attempts = sr.trunc_normal(n, first, bound, seed, stream, step or 0, sm.TN_CAP)
    print("STEP-BOUND trunc_normal bound %g: %d attempts, excluded share %.5f" % (bound, attempts, near.mean()))
    assert near.mean() <= 0.01 and attempts <= 255
    assert np.isfinite(z).all() and (bound <= 0 or np.abs(z).max() <= bound)
    # the moments of a standard normal cut at the bound
    if bound == 0:
        assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    if bound == 0.1:
        assert attempts > 12, "about 12 calls per group at acceptance 0.08"
    # another step word gives other numbers (what a dropped counter word would look like)
    z2, _, _ = sr.trunc_normal(min(n, 4096), first, bound, seed, stream, (step or 0) + 1, 0.0)
    assert np.abs(z2 - z[:z2.size]).max() > 10 * sm.TN_CAP


def test_slot_fold_rules():
    inf, nan, big = np.inf, np.nan, sr.INT_MAX
    pb = np.array([[-1, -1, -3], [-3, -1, -1], [-inf, -inf, -inf], [-inf, -inf, -inf], [nan, -5, nan], [nan, nan, nan], [-2, nan, -1]], dtype=np.float32)
    pi = np.array([[9, 4, 1], [1, 9, 4], [7, 3, 5], [big, big, big], [1, 8, 2], [4, 5, 6], [3, 0, 6]], dtype=np.int32)
    assert sr.fold_slots(pb, pi).tolist() == [4, 4, 3, 0, 8, 0, 6]
    pb2, pi2 = sm.slot_partials(15, sm.NSLOTS_V, 729, 7 + sm.NSLOTS_V)
    f = sr.fold_slots(pb2, pi2)
    assert f[0] == 3 and f[1] == pi2[1].min() and f[2] == 0 and f[4] == 0 and f[5] == pi2[5, -1]


def test_split_table_parts_add_up():
    t = sr.rng(1).standard_normal((5, 128)).astype(np.float32)
    p = sr.split_table(t, 5, 128, 8)
    hi, hi2, lo = (sr.from_panel(p[4 * i:4 * i + 4], 8) for i in range(3))
    assert np.array_equal(hi, hi2) and np.all(hi[5:] == 0) and np.all(lo[5:] == 0)
    assert np.abs((hi[:5].astype(np.float64) + lo[:5]) - t).max() <= 2.0 ** -17 * np.abs(t).max()
    assert np.array_equal(sr.from_panel(sr.to_panel(t, 7), 5), t) and np.array_equal(sr.from_panel(sr.pack_panel(t[:, :100], 6, 128), 5, 100), sr.bf16_round(t[:, :100]))


def test_exact_update_reference_properties():
    """the numpy update at the schedule's edges: sigma 0 at t = 0 (noise has no effect), the clip, anchoring"""
    g = sr.rng(2)
    x0, xt, nz, xs = (g.standard_normal((2, 3, 4)).astype(np.float32) * 2 for _ in range(4))
    for kind in ("p", "ddim"):
        tab = sr.coef_table(kind, 0.5 if kind == "ddim" else 0.0)
        assert tab[0, 2] == 0 and tab[1999, 2] > 0
        s0, p0, _ = sr.step_update(x0, xt, nz, tab[[0, 0]], 1, kind == "ddim")
        s1, _, _ = sr.step_update(x0, xt, None, tab[[0, 0]], 1, kind == "ddim")
        assert np.array_equal(s0, s1) and np.abs(p0).max() == 1.0
        m = np.array([[0, 1, 1], [1, 0, 1]], dtype=np.int32)
        s2, _, _ = sr.step_update(x0, xt, nz, tab[[1999, 1000]], 0, kind == "ddim", m, xs)
        assert np.array_equal(s2[0, 0], xs[0, 0]) and np.array_equal(s2[1, 1], xs[1, 1]) and not np.array_equal(s2[0, 1], xs[0, 1])


# ------------------------------------------------------------------------------------------------------------------ half-bound restatements
@pytest.mark.parametrize("V,E", sm.SQNORM_CASES)
def test_row_sqnorm_emulation_within_half_the_bound(V, E):
    t = sm.sqnorm_inputs(V, E)
    got = (t * t).sum(1, dtype=np.float32)
    assert sr.ratio(got, *sr.row_sqnorm(t)) <= HALF
    if E > 1:
        assert sr.ratio(got - t[:, -1] ** 2, *sr.row_sqnorm(t)) > 1.0      # (sees one element missing)


@pytest.mark.parametrize("dim,dtype", sm.TE_CASES, ids=lambda v: str(v))
def test_timestep_embedding_emulation_within_half_the_bound(dim, dtype):
    got = sr.timestep_embedding_emulate(sm.TE_T, dim)
    ref = sr.timestep_embedding(sm.TE_T, dim, dtype)
    assert within(got, ref, dtype)
    # a frequency taken at k + 1 is outside it
    wrong = sr.timestep_embedding_emulate(sm.TE_T * np.float32(np.exp(-np.log(10000.0) / (dim // 2))), dim)
    assert sr.ratio(wrong, *ref) > 1.0


def _one_pass(v, gamma, beta, eps):
    """E[x^2] - mean^2 in float32: what the cancellation rows are there to expose"""
    f = np.float32
    v = v.astype(f)
    mean = v.mean(1, keepdims=True, dtype=f)
    var = np.maximum((v * v).mean(1, keepdims=True, dtype=f) - mean * mean, f(0))
    return (v - mean) / np.sqrt(var + f(eps)) * gamma + beta


@pytest.mark.parametrize("case", sm.LN_CASES, ids=sm._ln_id)
def test_layernorm_emulation_within_half_the_bound(case):
    H, dtype, cancel = case
    for rows in sm.LN_ROWS:
        x, gamma, beta = sr.ln_inputs(rows, H, dtype, H * 3 + rows, cancel)
        ref = sr.layernorm(x, gamma, beta, sm.EPS, dtype, sr.ln_depth(H))
        assert within(sr.layernorm_emulate(x, gamma, beta, sm.EPS), ref, dtype), (rows, sr.ratio(sr.layernorm_emulate(x, gamma, beta, sm.EPS), *ref))
        if cancel and dtype == F32 and rows > 1:
            assert sr.ratio(_one_pass(x, gamma, beta, sm.EPS), *ref) > 1.0
        if rows > 1:    # the neighbouring row's statistics are outside it
            y = sr.layernorm_emulate(x, gamma, beta, sm.EPS)
            xs = np.roll(x, 1, axis=0)
            wrong = (x - xs.mean(1, keepdims=True)) / xs.std(1, keepdims=True) * gamma + beta
            assert sr.ratio(wrong, *ref) > 1.0 and y.shape == wrong.shape


@pytest.mark.parametrize("case", sm.LN_ADD_CASES, ids=sm._ln_add_id)
def test_add_pos_time_layernorm_emulation_within_half_the_bound(case):
    H, xt, ot, rows_given, cancel = case
    for B, L in sm.LN_ADD_BL:
        x, gamma, beta, pos, emb_t, rows_of = sm.ln_add_inputs(B, L, H, xt, rows_given, cancel, H + B * L)
        v = sr.add_pos_time(x, pos, emb_t, rows_of, L)
        ref = sr.layernorm(v, gamma, beta, sm.EPS, ot, sr.ln_depth(H))
        assert within(sr.layernorm_emulate(v, gamma, beta, sm.EPS), ref, ot)
        if B > 1 and rows_given:     # emb_row ignored (row b of emb_t instead) is outside it
            wrong = sr.add_pos_time(x, pos, emb_t, np.arange(B, dtype=np.int32), L)
            assert sr.ratio(sr.layernorm_emulate(wrong, gamma, beta, sm.EPS), *ref) > 1.0


@pytest.mark.parametrize("case", sm.PANEL_CASES + sm.PANEL16_DBG_CASES, ids=sm._panel_id)
def test_layernorm_panel_emulation_within_half_the_bound(case):
    H, form, add, rows_given = case
    for B, L in (sm.PANEL_ADD_BL if add else [(r, 1) for r in sm.PANEL_ROWS]):
        rows = B * L
        xt = F32 if add == "f32" else BF16
        x, gamma, beta, pos, emb_t, rows_of = sm.ln_add_inputs(B, L, H, xt, rows_given, 0, H * 5 + rows)
        v = sr.add_pos_time(x, pos, emb_t, rows_of, L) if add else x
        assert within(sr.layernorm_emulate(v, gamma, beta, sm.EPS, order="numpy"), sr.layernorm(v, gamma, beta, sm.EPS, BF16, sr.ln_depth(H, form)), BF16)


# ------------------------------------------------------------------------------------------------------------------ argbest
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,V,E", sm.MFMA_CASES)
def test_argbest_inputs_keep_the_near_tie_class_small(n, V, E, mode):
    """the float32 restatement's scores within half the per-row bound, its choice passes the margin rule, and at most 1 % of the rows are
    near ties; the planted duplicates are really chosen (so the first-copy rule has something to check)"""
    x, table, bias, tnorm, first_of = sm.arg_inputs(n, V, E)
    scores, bound = sr.round_scores(x, table, tnorm) if mode == 0 else sr.logit_scores(x, table, bias)
    got, s32 = sr.vocab_argmax_emulate(x, table, tnorm if mode == 0 else bias, mode)
    assert np.all(np.abs(s32.astype(np.float64) - scores) <= HALF * bound[:, None])
    near, bad = sr.argbest_check(scores, bound, got, first_of)
    assert not bad, bad
    assert near <= sm.NEAR_CAP * n, (near, n)
    dup = int((first_of != np.arange(V)).sum())
    if mode == 0 and E >= 16 and dup and n >= 2 * dup:
        later = np.nonzero(first_of != np.arange(V))[0]
        assert set(first_of[later]) <= set(got.tolist()), "no row rounds to a duplicated table row"
        # ... and the LAST index of the tie is refused
        last = (s32.shape[1] - 1) - s32[:, ::-1].argmax(1)
        assert sr.argbest_check(scores, bound, last, first_of)[1]


# ------------------------------------------------------------------------------------------------------------------ head and tail
@pytest.mark.parametrize("case", sm.HEAD_CASES, ids=lambda c: "H%d-E%d-Epad%d-embrow%d" % c)
def test_head_emulation_within_half_the_bound(case):
    H, E, Ep, rows_given = case
    for B, L in sm.HEAD_BL:
        x, w0, b0, w2, b2, pos, emb_t, rows_of, gamma, beta = sm.head_inputs(H, E, Ep, B, L, rows_given)
        ref = sr.head(x, Ep, w0, b0, w2, b2, pos, emb_t, rows_of, L, gamma, beta, sm.EPS)
        xb = np.zeros((B * L, Ep), dtype=np.float32)
        xb[:, :E] = sr.bf16_round(x)
        y2 = sr.dense_emulate(xb, w0, b0, w2, b2)
        v = sr.add_pos_time(y2, pos, emb_t, rows_of, L)
        # its own bf16 intermediate (roundings may flip): the whole bound; the reference's intermediate: half of the bound without flips
        assert sr.ratio(sr.q(sr.layernorm_emulate(v, gamma, beta, sm.EPS, order="numpy"), BF16), *ref) <= 1.0
        v0 = sr.add_pos_time(sr.dense_emulate(xb, w0, b0, w2, b2, own_h=False), pos, emb_t, rows_of, L)
        assert within(sr.layernorm_emulate(v0, gamma, beta, sm.EPS, order="numpy"),
                      sr.head(x, Ep, w0, b0, w2, b2, pos, emb_t, rows_of, L, gamma, beta, sm.EPS, flips=False), BF16)
        if B > 1:      # batch item b + 1's time row is outside it
            wrong = sr.add_pos_time(y2, pos, emb_t, np.roll(rows_of, 1), L)
            assert sr.ratio(sr.layernorm_emulate(wrong, gamma, beta, sm.EPS, order="numpy"), *ref) > 1.0


@pytest.mark.parametrize("H,E", sm.TAIL_CASES)
def test_tail_emulation_within_half_the_bound(H, E):
    for rows in sm.TAIL_ROWS:
        X, w0, b0, w2, b2 = sm.tail_inputs(H, E, rows)
        ref = sr.tail(X, w0, b0, w2, b2)
        y = sr.dense_emulate(X, w0, b0, w2, b2)
        assert sr.ratio(y, *ref) <= 1.0
        assert sr.ratio(sr.dense_emulate(X, w0, b0, w2, b2, own_h=False), *sr.tail(X, w0, b0, w2, b2, flips=False)) <= HALF
        assert sr.ratio((y * y).sum(1, dtype=np.float32), *sr.row_sqnorm(y)) <= HALF
        assert sr.ratio(y + np.float32(0.01) * np.abs(y), *ref) > 1.0       # (a 1 % error is outside it)
        for V in sorted({v for h, v in sm.ROUND_ONLY_CASES if h == H} if E == 128 else ()):
            # the rounding inside the tail: the near-tie share of the split-bf16 scores on these rows
            scores, bound = sr.round_scores(y, sm.round_table(H, V, rows), None, split=True)
            near, bad = sr.argbest_check(scores, bound, scores.argmax(1))
            assert not bad and near <= sm.NEAR_CAP * rows, (H, V, near, rows)
