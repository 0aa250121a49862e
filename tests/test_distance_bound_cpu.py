"""The distance-logit matrix's bounds hold for plain float32 arithmetic (CPU): each kernel of csrc/distance_logits.hip and the mode-2
argmax of csrc/rounding.hip restated in float32 numpy (tests/distance_ref.py: *_emulate - the kernels' formula order, numpy's summation
order) stays within HALF of the per-element bound of its float64 reference, on every case of tests/test_distance_matrix_gpu.py's matrix
(same functions, same seeds).  A bound this restatement could not meet with that margin would be wrong; what it does not contain - the
exact-fp32 MFMA's and the wave reductions' summation orders, the device's expf / logf / sqrtf - is what the matrix measures on the GPU.

It also holds the matrix's two caps as CONDITIONS on the inputs (distance_ref.CAP): at most 1 % of a case's elements are clamp-uncertain
and at most 1 % of its rows low-margin, and the float32 restatement alone agrees with the float64 argmax on every other row - so the
seeds of distance_ref.case_inputs leave the GPU comparison nearly everything to compare."""
import numpy as np
import pytest

import distance_ref as dr

HALF = 0.5
CASES = [(V, E) for V, _ in dr.VS for E in dr.ES]


def capped(flags):
    """at most CAP of the flags set"""
    return int(flags.sum()) <= dr.CAP * flags.size


@pytest.mark.parametrize("V,E", CASES)
def test_float32_restatement_within_half_the_bounds(V, E):
    for N in dr.NS:
        W, x, ids, g = dr.case_inputs(V, E, N)
        dots, wn, xn = dr.dots_emulate(x, W)
        ref, sc = dr.ce_fwd(x, W, ids)
        s, e_s, d2, delta, unc = sc
        # d2 and the score themselves
        assert dr.ratio(dr.d2_emulate(dots, wn, xn), d2, delta) <= HALF, (N, "d2")
        r_s = dr.ratio(dr.scores_emulate(dots, wn, xn), s, e_s)
        lse, nll = dr.ce_fwd_emulate(dots, wn, xn, ids)
        r_l, r_n = dr.ratio(lse, *ref["lse"]), dr.ratio(nll, *ref["nll"])
        # backward, given the reference's lse as fp32 (what the GPU case feeds the kernel)
        lse32 = ref["lse"][0].astype(np.float32)
        (G, e_G), _ = dr.ce_bwd(x, W, ids, lse32, g, sc)
        Gg, dxn, dwn = dr.ce_bwd_emulate(dots, wn, xn, ids, lse32, g)
        r_g = dr.ratio(np.where(unc, 0.0, Gg), G, e_G)
        r_x = dr.ratio(dxn, *dr.g_sums(G, e_G, unc, Gg, 1))
        r_w = dr.ratio(dwn, *dr.g_sums(G, e_G, unc, Gg, 0))
        print("DISTANCE-BOUND V=%d E=%d N=%d  s %.3f lse %.3f nll %.3f G %.3f d_xn %.3f d_wn %.3f  uncertain %d / %d"
              % (V, E, N, r_s, r_l, r_n, r_g, r_x, r_w, unc.sum(), unc.size))
        assert max(r_s, r_l, r_n, r_g, r_x, r_w) <= HALF, N
        assert np.isfinite(Gg).all() and np.all(Gg[dr.d2_emulate(dots, wn, xn) <= 0] == 0)
        assert capped(unc), (N, int(unc.sum()))
        # every exact table row of the case is among the uncertain elements (float64 d2 == 0), and nothing else at these inputs
        assert int(unc.sum()) == int((d2 == 0).sum())
        idx, safe = dr.argmax(x, W, sc)
        assert capped(~safe), (N, int((~safe).sum()))
        got = dr.scores_emulate(dots, wn, xn).argmax(1)
        assert np.array_equal(got[safe], idx[safe])


def test_sqnorm_backward_bound():
    r = dr.rng(3)
    x = r.standard_normal((37, 65)).astype(np.float32)
    c = r.standard_normal(37).astype(np.float32)
    for c_scale in (1.0, -0.5):
        got = np.float32(2.0) * (np.float32(c_scale) * c)[:, None] * x
        assert dr.ratio(got, *dr.sqnorm_bwd(x, c, c_scale)) <= HALF


def test_tie_inputs_have_exact_ties_and_a_clear_margin_to_the_rest():
    """the duplicated rows score bit for bit the same in float32 as well, the first of a pair is the float64 argmax, and the best of all
    OTHER rows lies further off than twice the score bound - so the kernel's answer on these rows is decided by its tie rule alone"""
    for V, E in ((729, 32), (97, 128), (65, 500)):
        W, x, first = dr.tie_inputs(V, E, 70)
        sc = dr.scores(x, W)
        s, e_s = sc[0], sc[1]
        assert np.array_equal(s.argmax(1), first)
        twin = np.array([np.flatnonzero((W == W[f]).all(1))[-1] for f in first])
        assert np.all(twin > first) and np.array_equal(s[np.arange(70), twin], s[np.arange(70), first])
        rest = s.copy()
        rest[np.arange(70), first] = -np.inf
        rest[np.arange(70), twin] = -np.inf
        assert np.all(s[np.arange(70), first] - rest.max(1) > 2 * e_s.max(1))
        dots, wn, xn = dr.dots_emulate(x, W)
        assert np.array_equal(dr.scores_emulate(dots, wn, xn).argmax(1), first)


def test_the_bound_sees_a_wrong_formula():
    """not a multiple of the output: the NLL of mode-1 logits (x.W), a score without the square root and a gradient without the clamp's
    zero all fall outside"""
    V, E, N = 97, 32, 65
    W, x, ids, g = dr.case_inputs(V, E, N)
    dots, wn, xn = dr.dots_emulate(x, W)
    ref, sc = dr.ce_fwd(x, W, ids)
    mx = dots.max(1, keepdims=True)
    lse1 = (mx + np.log(np.exp(dots - mx).sum(1, keepdims=True)))[:, 0]
    assert dr.ratio(lse1 - dots[np.arange(N), ids], *ref["nll"]) > 1.0
    assert dr.ratio(-np.maximum(dr.d2_emulate(dots, wn, xn), 0), sc[0], sc[1]) > 1.0
    lse32 = ref["lse"][0].astype(np.float32)
    (G, e_G), unc = dr.ce_bwd(x, W, ids, lse32, g, sc)
    Gg = dr.ce_bwd_emulate(dots, wn, xn, ids, lse32, g)[0]
    assert dr.ratio(np.where(unc, 0.0, 2 * Gg), G, e_G) > 1.0
