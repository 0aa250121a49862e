"""Parity matrix of the distance-logit kernels (csrc/distance_logits.hip; vocab_argmax_kernel<2> of csrc/rounding.hip): the entry points
mh_distance_ce_fwd / mh_distance_ce_bwd / mh_sqnorm_bwd / mh_distance_argmax called through the library's ABI against the float64 references
of tests/distance_ref.py, EVERY element of EVERY output, |got - ref| <= bound per element (the bounds are derived there;
tests/test_distance_bound_cpu.py holds a float32 restatement to half of them and the inputs to the two caps).

Cases: V in {729 (pitch 768), 97 (128), 64 (64: no padding column), 65 (128)} x E in {32, 128, 500} (the GEMM's operands padded to 64 /
128 / 512 columns) as the parametrisation, N in {1, 63, 64, 65, 200} inside each (a wave per row, four rows per block: ragged last
blocks, blocks whose last waves own no row).  Rows: random positions, positions that ARE a table row with the id on that row and on
another one (the clamp active on and off the target), and W[id] + 0.01 noise (the decoder-NLL regime of _get_x_start, where d2 cancels
to 1e-3 of its terms).  g has zeros and both signs.  The product `dots` comes from the exact-fp32 GEMM as the tape makes it, and its
padding columns are then filled with 3e30: a padding column read into a maximum or a sum would show in every row.

Rules: every output starts as NaN and is larger than the kernel may write; what lies behind the documented output must still be NaN;
d_dots' padding columns must be exactly 0; clamp-uncertain elements (float64 d2 <= delta) are left out of the element-wise backward
comparison and enter the row / column sums with the kernel's own value; where the kernel's own fp32 d2 (the same expression on the same
product, evaluated on the host: bit for bit) is <= 0 the gradient must be exactly 0; every gradient is finite.

Worst |got - ref| / bound over all cases, measured on an MI355X (every case prints its own DISTANCE-MATRIX line): lse 0.21, nll 0.16,
G 0.07, d_xn 0.05, d_wn 0.05, dW and dx 0.20 (one rounding against a bound of one rounding plus the output term)."""
import numpy as np
import pytest
import torch

import distance_ref as dr

pytestmark = pytest.mark.gpu

from musediffusion_amd import ops, training  # noqa: E402
from musediffusion_amd._lib import MH_ERR_INVALID, MH_F32, check, current_stream, lib, ptr  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SLACK = 256
CASES = [(V, ld, E) for V, ld in dr.VS for E in dr.ES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def ints(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def nans(n):
    return torch.full((int(n) + SLACK,), NAN, dtype=torch.float32, device=DEV)


def read(t, n, what):
    a = t.cpu().numpy()
    assert np.isnan(a[n:]).all(), "%s: written behind its %d elements" % (what, n)
    return a[:n]


def run(fn, *args):
    check(fn(*args, current_stream()), fn.__name__)


def product(x, W, V, ld):
    """x W^T on the exact-fp32 GEMM into a [N, ld] buffer whose padding columns then hold PAD_FILL; |W_v|^2, |x_n|^2"""
    N, E = x.shape
    Ep = ops.pad64(E)
    xd, Wd = dev(x), dev(W)
    buf = torch.zeros(N * ld + SLACK, dtype=torch.float32, device=DEV)
    dots = buf[:N * ld].view(N, ld)
    ops.gemm_bias_act(ops.cast_pad(xd, Ep, MH_F32), ops.cast_pad(Wd, Ep, MH_F32), None, None, None, MH_F32, out_f32=True, N=V, K=Ep, out=dots)
    dots[:, V:] = dr.PAD_FILL
    return xd, Wd, dots, ops.row_sqnorm(Wd), ops.row_sqnorm(xd)


def worst(case, name, got, ref, bound, out):
    r = dr.ratio(got, ref, bound)
    out[name] = max(out.get(name, 0.0), r)
    assert r <= 1.0, "%s %s: |got - ref| / bound = %.3f" % (case, name, r)


@pytest.mark.parametrize("V,ld,E", CASES)
def test_distance_ce_forward_and_backward_against_float64(V, ld, E):
    seen = {}
    for N in dr.NS:
        case = "V=%d ld=%d E=%d N=%d" % (V, ld, E, N)
        W, x, ids, g = dr.case_inputs(V, E, N)
        ref, sc = dr.ce_fwd(x, W, ids)
        xd, Wd, dots, wn, xn = product(x, W, V, ld)
        idd = ints(ids)
        # ---- forward
        nll, lse = nans(N), nans(N)
        run(lib().mh_distance_ce_fwd, ptr(dots), ld, ptr(wn), ptr(xn), ptr(idd), ptr(nll), ptr(lse), N, V)
        worst(case, "lse", read(lse, N, "lse"), *ref["lse"], seen)
        worst(case, "nll", read(nll, N, "nll"), *ref["nll"], seen)
        # ---- backward, given the reference's lse (fp32)
        lse32 = ref["lse"][0].astype(np.float32)
        (G, e_G), unc = dr.ce_bwd(x, W, ids, lse32, g, sc)
        assert int(unc.sum()) <= dr.CAP * unc.size
        d_dots, d_xn = nans(N * ld), nans(N)
        lsed, gd = dev(lse32), dev(g)            # (named: a temporary's block is handed to the next allocation before the kernel runs)
        run(lib().mh_distance_ce_bwd, ptr(dots), ld, ptr(wn), ptr(xn), ptr(idd), ptr(lsed), ptr(gd), ptr(d_dots), ptr(d_xn), N, V)
        dd = read(d_dots, N * ld, "d_dots").reshape(N, ld)
        assert np.all(dd[:, V:] == 0), case + ": padding columns of d_dots"
        assert np.isfinite(dd).all(), case
        Gg = -0.5 * dd[:, :V].astype(np.float64)
        worst(case, "G", np.where(unc, 0.0, Gg), G, e_G, seen)
        d2_dev = dr.d2_emulate(dots[:, :V].cpu().numpy(), wn.cpu().numpy(), xn.cpu().numpy())
        clamped = d2_dev <= 0
        assert np.all(dd[:, :V][clamped] == 0), case + ": gradient where the clamp is active"
        assert np.all(clamped <= unc), case + ": the kernel clamps an element the reference holds certain"
        worst(case, "d_xn", read(d_xn, N, "d_xn"), *dr.g_sums(G, e_G, unc, Gg, 1), seen)
        # ---- d_wn = -1/2 colsum(d_dots), on to x and W through mh_sqnorm_bwd
        colsum = training._col_sum(d_dots[:N * ld].view(N, ld), N, V, MH_F32)
        cs = colsum.cpu().numpy()
        worst(case, "d_wn", -0.5 * cs.astype(np.float64), *dr.g_sums(G, e_G, unc, Gg, 0), seen)
        dW = nans(V * E)
        run(lib().mh_sqnorm_bwd, ptr(Wd), E, ptr(colsum), -0.5, ptr(dW), E, V, E)
        worst(case, "dW", read(dW, V * E, "dW").reshape(V, E), *dr.sqnorm_bwd(W, cs, -0.5), seen)
        ldo = E + 3
        dx = nans(N * ldo)
        run(lib().mh_sqnorm_bwd, ptr(xd), E, ptr(d_xn), 1.0, ptr(dx), ldo, N, E)
        body = read(dx, N * ldo, "dx").reshape(N, ldo)
        assert np.isnan(body[:, E:]).all(), case + ": pitch columns of dx"
        worst(case, "dx", body[:, :E], *dr.sqnorm_bwd(x, d_xn[:N].cpu().numpy(), 1.0), seen)
    print("DISTANCE-MATRIX V=%d ld=%d E=%d  " % (V, ld, E) + "  ".join("%s %.3f" % kv for kv in seen.items()))


@pytest.mark.parametrize("V,ld,E", CASES)
def test_distance_argmax_against_float64(V, ld, E):
    for N in dr.NS:
        W, x, ids, g = dr.case_inputs(V, E, N)
        idx, safe = dr.argmax(x, W)
        assert int((~safe).sum()) <= dr.CAP * N
        out = torch.full((N + SLACK,), -7, dtype=torch.int32, device=DEV)
        xd, Wd = dev(x), dev(W)
        wn = ops.row_sqnorm(Wd)
        run(lib().mh_distance_argmax, ptr(xd), ptr(Wd), ptr(wn), ptr(out), N, E, V)
        got = out.cpu().numpy()
        assert np.all(got[N:] == -7)
        assert np.array_equal(got[:N][safe], idx[safe]), (V, E, N)
        assert np.all((got[:N] >= 0) & (got[:N] < V))


@pytest.mark.parametrize("V,E", [(729, 32), (97, 128), (65, 500)])
def test_distance_argmax_returns_the_first_index_of_a_tie(V, E):
    """duplicated table rows score the same bit for bit: the lower index wins, across 64-row tiles and lanes (strict > in ascending v)"""
    N = 70
    W, x, first = dr.tie_inputs(V, E, N)
    xd, Wd = dev(x), dev(W)
    wn = ops.row_sqnorm(Wd)
    out = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    run(lib().mh_distance_argmax, ptr(xd), ptr(Wd), ptr(wn), ptr(out), N, E, V)
    assert np.array_equal(out.cpu().numpy(), first)


def test_bad_arguments_are_refused_before_any_launch():
    V, ld, E, N = 97, 128, 32, 5
    W, x, ids, g = dr.case_inputs(V, E, N)
    xd, Wd, dots, wn, xn = product(x, W, V, ld)
    for bad in (-1, V):
        b = ids.copy()
        b[3] = bad
        nll, lse, bd = nans(N), nans(N), ints(b)
        rc = lib().mh_distance_ce_fwd(ptr(dots), ld, ptr(wn), ptr(xn), ptr(bd), ptr(nll), ptr(lse), N, V, current_stream())
        assert rc == MH_ERR_INVALID
        assert "outside" in lib().mh_last_error().decode()
        torch.cuda.synchronize()
        assert torch.isnan(nll).all() and torch.isnan(lse).all()
    nll, lse, idd = nans(N), nans(N), ints(ids)
    assert lib().mh_distance_ce_fwd(ptr(dots), V - 1, ptr(wn), ptr(xn), ptr(idd), ptr(nll), ptr(lse), N, V, current_stream()) == MH_ERR_INVALID
    assert lib().mh_distance_ce_bwd(ptr(dots), V - 1, ptr(wn), ptr(xn), ptr(idd), ptr(lse), ptr(lse), ptr(nll), ptr(nll), N, V,
                                    current_stream()) == MH_ERR_INVALID
    assert lib().mh_sqnorm_bwd(ptr(xd), E - 1, ptr(xn), 1.0, ptr(nll), E, N, E, current_stream()) == MH_ERR_INVALID
    assert lib().mh_distance_argmax(ptr(xd), ptr(Wd), None, ptr(nll), N, E, V, current_stream()) == MH_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(nll).all() and torch.isnan(lse).all()
