"""Parity matrix of the training kernels (csrc/train.hip): every C entry point but the optimizer's three (mh_adamw_ema_step, mh_grad_norm,
mh_clip_grads: tests/test_optim_matrix_gpu.py, by the same rules) called through the library's ABI against a float64 reference
on the CPU (tests/train_ref.py), EVERY element of EVERY output, at the shapes where a streaming kernel goes wrong - a single lane in the
last 16-byte chunk column (H = 520, 1032), the four-chunk LayerNorm build (H > 1024), blocks and waves that own no row, the partial
fold's unrolled loop (more than 48 partials) and its tail, a second pass over the embedding columns (E > 256), the 32-chunk scatter,
pitches wider than the rows, pointers 4 bytes off a 16-byte boundary, and the second sweep of the grid-stride loops.

Rules of every case: inputs are rounded to their storage type first; every output and scratch buffer starts as NaN and is larger than the
kernel may write (pitch columns, rows behind the last, SLACK elements behind the end, the partial scratch of every block), and whatever
lies outside the documented output must still be NaN afterwards; the comparison is |got - ref| <= bound per element with the bounds of
tests/train_ref.py (derived from where the kernels round; tests/test_train_bound_cpu.py holds a float32 restatement to half of them); the
exact kernels (layout movers, the two adds) are compared bit for bit.  Most cases record their launch (tests/train_census.py) and assert
which kernel and path they ran, which is what tests/test_train_census_gpu.py's PARITY table rests on.

Wrap cases: tgrid() caps a grid-stride launch at 16384 blocks x 256 threads = 4 194 304 work items.  The scalar kernels (one element per
work item) wrap at 4 194 305 elements and get one case each at 16384 x 256 + 257 elements (scatter_rows_final_kernel: a 16 x 262161 table):
act_fwd / act_bwd, add_inplace and add_pos_time in both storage types, head_permute_kernel in both, sqdiff_bwd, scale_rows,
scatter_rows_final.  The 8-wide kernels (add_pos_time8, head_permute8, repack_panel: 8 elements per work item) wrap only above 33.5 M
elements and sum_slices_kernel (4 per work item) above 16.7 M; the product does not reach either at the shapes bench.py runs (its largest
split-K fold is 512 x 2048 = 1 M floats), and those cases are not built.

Worst |got - ref| / bound per output, measured on an MI355X over all cases of a test (every case prints its own TRAIN-MATRIX line):

    output                                   bf16    fp32
    LayerNorm backward  dx                   0.99    0.06
                        dropped copy         0.58    0.06        (its bound allows the kernel's own rounding of dx to flip: a whole ulp)
                        dgamma               0.01    0.09        (fp32 sums whatever the storage type; the bf16 cases' dy is coarser)
                        dbeta                0.00    0.19
    column sums (and the split-K fold)         -     0.24
    scatter-add         table                  -     0.31
    cross-entropy       lse | loss             -     0.15 | 0.40
                        dlogits              1.00    0.23
    squared error       mean | da | db         -     0.09 | 0.32 | 0.44
    scale rows          dst                    -     0.20
    row softmax         p | ds               0.95 | 0.98    0.19 | 0.10
    activations         y | dx               0.98 | 1.00    0.33 | 0.50

The bf16 column is the output rounding itself: bf16 keeps 8 significant bits, so rounding to nearest costs up to 2^-8 |ref|, the whole of the
bound's output term (0.996 is the worst seen, an element just above a power of two), and the arithmetic in front of it shows in the fp32
column.  The fp32 bounds are worst-case (n u per sum), hence the distance.  No output needed a term beyond the derived bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_census as gc
import train_census as tc
import train_ref as tr

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import check, current_stream, lib  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SLACK = 256
WRAP = 16384 * 256 + 257
TD = {tr.BF16: torch.bfloat16, tr.F32: torch.float32}
TNAME = {tr.BF16: "bf16", tr.F32: "float"}
DT = pytest.mark.parametrize("dtype", [tr.BF16, tr.F32], ids=["bf16", "f32"])


# ------------------------------------------------------------------------------------------------------------------ buffers
def dev(a, dtype=tr.F32):
    """stored values (float32 numpy, already rounded) -> device tensor of the storage type"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t.to(TD[dtype]) if dtype == tr.BF16 else t


def ints(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def nans(n, dtype=tr.F32):
    return torch.full((int(n) + SLACK,), NAN, dtype=TD[dtype], device=DEV)


def host(t):
    return t.float().cpu().numpy()


def read(t, n, what):
    """the first n elements of a NaN-initialised buffer; everything behind them must still be NaN"""
    a = host(t)
    assert np.isnan(a[n:]).all(), "%s: written behind its %d elements" % (what, n)
    return a[:n]


def read_pitched(t, rows, cols, ld, what):
    """[rows, cols] out of a NaN-initialised buffer with pitch ld; pitch columns and the tail must still be NaN"""
    a = host(t)
    body = a[:rows * ld].reshape(rows, ld)
    assert np.isnan(body[:, cols:]).all() and np.isnan(a[rows * ld:]).all(), "%s: written outside its [%d, %d] (pitch %d)" % (what, rows, cols, ld)
    return body[:, :cols]


def fill_pitched(t, a, ld, dtype):
    rows, cols = a.shape
    t[:rows * ld].view(rows, ld)[:, :cols] = dev(a, dtype)


def run(fn, *args):
    check(fn(*args, current_stream()), fn.__name__)


def compare(case, name, got, pair):
    """one output against (ref, bound), every element; prints the worst err / bound (the module docstring's table)"""
    ref, bound = pair
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), "%s %s: %d elements never written (still NaN) or not finite, first at %s" % (
        case, name, int(bad.sum()), np.unravel_index(int(np.argmax(bad)), ref.shape))
    print("TRAIN-MATRIX %s %s %.3f" % (case, name, tr.ratio(got, ref, bound)))
    err = np.abs(got - ref)
    out = err > bound
    if out.any():
        i = np.unravel_index(int(np.argmax(err - bound)), ref.shape)
        pytest.fail("%s %s: %d of %d elements outside their bound; worst at %s: got %.9g ref %.9g (bound %.3g); first bad rows %s"
                    % (case, name, int(out.sum()), out.size, i, got[i], ref[i], bound[i], sorted(set(np.nonzero(out)[0].tolist()))[:8]))


def exact(case, name, got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), "%s %s: %d of %d elements differ, first at %s" % (case, name, int(diff.sum()), diff.size,
                                                                           np.unravel_index(int(np.argmax(diff)), diff.shape))


def rejected(fn, *args):
    """an argument check that returns before any launch"""
    assert fn(*args, current_stream()) != 0
    assert lib().mh_last_error()


# ------------------------------------------------------------------------------------------------------------------ LayerNorm backward
# (H, rows, n_partial, dtype, dgamma | dbeta adjacent, accumulate, eps, entry, p, always, panel)
LN_CASES = [
    (8, 1, 1, tr.BF16, 1, 0, 1e-12, "plain", 0.0, 0, 0),
    (8, 5, 3, tr.F32, 0, 1, 1e-5, "plain", 0.0, 0, 0),
    (8, 7, 1, tr.F32, 1, 0, 1e-5, "ex", 0.1, 1, 0),
    (128, 263, 64, tr.BF16, 1, 0, 1e-12, "drop", 0.1, 0, 0),
    (128, 4 * 1024 + 3, 1024, tr.BF16, 0, 0, 1e-5, "ex", 0.1, 0, 1),
    (128, 5, 65, tr.F32, 1, 1, 1e-12, "plain", 0.0, 0, 0),
    (128, 263, 65, tr.F32, 0, 0, 1e-5, "drop", 0.1, 0, 0),
    (512, 263, 64, tr.BF16, 1, 0, 1e-12, "ex", 0.1, 1, 1),
    (512, 263, 65, tr.BF16, 1, 0, 1e-5, "ex", 0.0, 1, 1),
    (520, 263, 65, tr.BF16, 1, 0, 1e-5, "ex", 0.0, 1, 0),
    (520, 15, 3, tr.F32, 0, 0, 1e-12, "ex", 0.1, 1, 0),
    (1024, 263, 64, tr.BF16, 0, 1, 1e-5, "ex", 0.0, 1, 1),
    (1024, 263, 65, tr.F32, 1, 0, 1e-12, "plain", 0.0, 0, 0),
    (1032, 263, 64, tr.BF16, 1, 0, 1e-5, "drop", 0.1, 0, 0),
    (1032, 1, 1024, tr.F32, 0, 0, 1e-12, "plain", 0.0, 0, 0),
    (2048, 4 * 64 + 3, 64, tr.BF16, 1, 1, 1e-5, "ex", 0.1, 0, 1),
    (2048, 5, 3, tr.F32, 1, 0, 1e-12, "ex", 0.0, 0, 0),
    (2048, 263, 1, tr.BF16, 0, 0, 1e-5, "plain", 0.0, 0, 0),
    (2048, 263, 65, tr.F32, 0, 1, 1e-5, "ex", 0.1, 1, 1),
]


def _ln_id(c):
    H, rows, P, dtype, adj, acc, eps, entry, p, always, panel = c
    return "H%d-r%d-P%d-%s-%s-acc%d-eps%g-%s-p%g-always%d-%s" % (H, rows, P, TNAME[dtype], "adjacent" if adj else "separate", acc, eps, entry, p,
                                                              always, "panel" if panel else "rows")


def ln_case_keys(case):
    """the census keys a LayerNorm case launches (asserted by the case itself)"""
    H, rows, P, dtype, adj, acc, eps, entry, p, always, panel = case
    second = entry != "plain" and (p > 0 or always)
    lnch = 1 if H <= 512 else (2 if H <= 1024 else 4)
    return [tc.ln_key(TNAME[dtype], lnch, second, panel, always, int(p > 0))] + [tc.fold_key(P, acc)] * (1 if adj else 2)


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm_backward(case):
    H, rows, P, dtype, adj, acc, eps, entry, p, always, panel = case
    name = _ln_id(case)
    x, dy, gamma, start_g, start_b = tr.ln_case_inputs(H, rows, P, acc, dtype)
    ref = tr.ln_bwd(x, dy, gamma, eps, dtype, start_g, start_b)
    xd, dyd, gd = dev(x, dtype), dev(dy, dtype), dev(gamma)
    dx, part = nans(rows * H, dtype), nans(2 * P * H)
    if adj:
        gb = nans(2 * H)
        pg, pb, bufs = gb.data_ptr(), gb.data_ptr() + 4 * H, [gb]
    else:
        bufs = [nans(H), nans(H)]
        pg, pb = bufs[0].data_ptr(), bufs[1].data_ptr()
    if acc:
        bufs[0][:H] = dev(start_g)
        if adj:
            bufs[0][H:2 * H] = dev(start_b)
        else:
            bufs[1][:H] = dev(start_b)
    seed, offset = 0x1234567 + H, 3 + rows
    drop = _lib.Dropout(p, seed, offset, None)
    ldm = (rows + 3) if panel else (H + 8 if entry == "ex" else H)
    n_m = (H // 32) * ldm * 32 if panel else rows * ldm
    dxm = nans(n_m, dtype) if entry != "plain" else None
    st = current_stream()

    def launch():
        if entry == "plain":
            check(lib().mh_layernorm_bwd(xd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), dx.data_ptr(), part.data_ptr(), P, pg, pb, acc, rows, H, eps,
                                         dtype, st), "mh_layernorm_bwd")
        elif entry == "drop":
            check(lib().mh_layernorm_bwd_drop(xd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), dx.data_ptr(), dxm.data_ptr(), C.byref(drop), part.data_ptr(),
                                              P, pg, pb, acc, rows, H, eps, dtype, st), "mh_layernorm_bwd_drop")
        else:
            check(lib().mh_layernorm_bwd_ex(xd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), dx.data_ptr(), dxm.data_ptr(), ldm, panel, always,
                                            C.byref(drop), part.data_ptr(), P, pg, pb, acc, rows, H, eps, dtype, st), "mh_layernorm_bwd_ex")
    keys = tc.keys_of(launch)
    second = entry != "plain" and (p > 0 or always)
    assert keys == ln_case_keys(case), keys
    compare(name, "dx", read(dx, rows * H, "dx"), ref["dx"])
    pa = read(part, 2 * P * H, "partial")
    assert np.isfinite(pa).all(), "a block left its partial row unwritten"
    if adj:
        gg = read(bufs[0], 2 * H, "dgamma | dbeta")
        got_g, got_b = gg[:H], gg[H:]
    else:
        got_g, got_b = read(bufs[0], H, "dgamma"), read(bufs[1], H, "dbeta")
    compare(name, "dgamma", got_g, ref["dgamma"])
    compare(name, "dbeta", got_b, ref["dbeta"])
    if dxm is None:
        return
    if not second:
        assert np.isnan(host(dxm)).all(), "no dropout and always = 0: the second output must stay untouched"
        return
    keep = gc.dense_keep(rows, H, p, seed, offset) if p > 0 else np.ones((rows, H), dtype=bool)
    if p > 0:
        assert 0.05 < 1.0 - keep.mean() < 0.2 or keep.size < 200
    m_ref = tr.ln_dropped(ref["dx"][0], ref["dx_arith"], keep, p, dtype)
    if panel:
        pan = read(dxm, n_m, "dropped copy").reshape(H // 32, ldm, 32)
        assert np.isnan(pan[:, rows:, :]).all(), "written into panel rows behind the last row"
        got_m = tr.from_panel(pan, rows)
    else:
        got_m = read_pitched(dxm, rows, H, ldm, "dropped copy")
    compare(name, "dx_dropped", got_m, m_ref)
    assert np.all(got_m[~keep] == 0)


def test_layernorm_backward_rejects_bad_shapes_before_any_launch():
    t = nans(4096, tr.BF16)
    f = nans(4096)
    a = (t.data_ptr(), t.data_ptr(), f.data_ptr(), t.data_ptr(), f.data_ptr())
    rejected(lib().mh_layernorm_bwd, *a, 1, f.data_ptr(), f.data_ptr(), 0, 4, 12, 1e-5, tr.BF16)          # H % 8
    rejected(lib().mh_layernorm_bwd, *a, 1025, f.data_ptr(), f.data_ptr(), 0, 4, 8, 1e-5, tr.BF16)       # n_partial > 1024
    rejected(lib().mh_layernorm_bwd, *a, 1, f.data_ptr(), f.data_ptr(), 0, 1, 2056, 1e-5, tr.BF16)       # H > 2048
    rejected(lib().mh_col_sum, t.data_ptr(), 8, 4, 8, 1, 32, f.data_ptr(), 1025, f.data_ptr(), 0, tr.BF16)
    assert np.isnan(host(t)).all() and np.isnan(host(f)).all()


# ------------------------------------------------------------------------------------------------------------------ column sums
# (cols, ld, rows, n_partial, batch, accumulate, dtype, 4-byte offset)
COLSUM_CASES = [
    (8, 8, 1, 1, 1, 0, tr.BF16, 0), (64, 64, 3, 16, 3, 1, tr.F32, 0), (520, 520, 1000, 17, 1, 0, tr.BF16, 0), (520, 520, 1000, 256, 3, 0, tr.F32, 0),
    (64, 64, 1000, 1024, 1, 1, tr.BF16, 0), (8, 8, 3, 64, 3, 1, tr.F32, 0), (1, 3, 3, 1, 1, 0, tr.BF16, 0), (63, 64, 1000, 64, 3, 0, tr.F32, 0),
    (65, 65, 1000, 65, 1, 1, tr.BF16, 0), (729, 731, 1000, 1024, 1, 0, tr.F32, 0), (64, 67, 3, 17, 3, 0, tr.BF16, 0), (729, 736, 1, 256, 3, 1, tr.BF16, 0),
    (1, 1, 1000, 16, 1, 0, tr.F32, 0), (65, 68, 3, 65, 3, 1, tr.F32, 0), (64, 64, 1000, 16, 1, 0, tr.F32, 1), (520, 520, 3, 65, 3, 1, tr.F32, 1),
]


def _colsum_id(c):
    return "c%d-ld%d-r%d-P%d-b%d-acc%d-%s%s" % (*c[:6], TNAME[c[6]], "-offset" if c[7] else "")


def colsum_case_keys(case):
    cols, ld, rows, P, batch, acc, dtype, off = case
    vec = 8 if dtype == tr.BF16 else 4
    wide = cols % vec == 0 and ld % vec == 0 and not off
    return ["%s<%s>" % ("colsum8_partial_kernel" if wide else "colsum_partial_kernel", TNAME[dtype]), tc.fold_key(P, acc)]


@pytest.mark.parametrize("case", COLSUM_CASES, ids=_colsum_id)
def test_column_sums(case):
    cols, ld, rows, P, batch, acc, dtype, off = case
    name = "colsum c%d ld%d r%d P%d b%d" % (cols, ld, rows, P, batch)
    flat, stride, x, start = tr.colsum_inputs(cols, ld, rows, P, batch, acc, dtype)
    buf = torch.empty(batch * stride + 1, dtype=TD[dtype], device=DEV)
    buf[off:off + batch * stride] = dev(flat, dtype)
    xin = buf[off:]
    assert xin.data_ptr() % 16 == (4 if off else 0)
    part, out = nans(batch * P * cols), nans(batch * cols)
    if acc:
        out[:batch * cols] = dev(start.reshape(-1))
    keys = tc.keys_of(lambda: run(lib().mh_col_sum, xin.data_ptr(), ld, rows, cols, batch, stride, part.data_ptr(), P, out.data_ptr(), acc, dtype))
    assert keys == colsum_case_keys(case), keys
    assert np.isfinite(read(part, batch * P * cols, "partial")).all()
    compare(name, "out", read(out, batch * cols, "out"), tr.col_sum(x, start))


# ------------------------------------------------------------------------------------------------------------------ embedding scatter-add
# (the last: V E = 16 x 262161 > 16384 x 256, the second sweep of scatter_rows_final_kernel's grid-stride loop; 1025 column passes of the partial kernel)
SCATTER_CASES = [(1, 16, 8, 0), (257, 128, 729, 0), (8191, 128, 729, 1), (8192 + 37, 128, 729, 0), (3000, 260, 13, 0), (3000, 516, 9, 0),
                 (5, (WRAP + 15) // 16, 16, 0)]


@pytest.mark.parametrize("n,E,V,clamp", SCATTER_CASES)
def test_scatter_add_rows(n, E, V, clamp):
    src, ids, table = tr.scatter_inputs(n, E, V, clamp)
    nbytes = int(lib().mh_scatter_add_rows_workspace_bytes(E, V))
    assert nbytes == 32 * V * E * 4
    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    tab = nans(V * E)
    tab[:V * E] = dev(table.reshape(-1))
    sd, idd = dev(src), ints(ids)
    keys = tc.keys_of(lambda: run(lib().mh_scatter_add_rows, sd.data_ptr(), idd.data_ptr(), tab.data_ptr(), n, E, V, ws.data_ptr(), nbytes))
    chunks = 32 if n >= 8192 else (n + 255) // 256
    assert keys == [tc.scatter_key(chunks, E), "scatter_rows_final_kernel"], keys
    w = host(ws).reshape(32, V * E)
    assert np.isfinite(w[:chunks]).all() and np.isnan(w[chunks:]).all()
    compare("scatter n%d E%d V%d" % (n, E, V), "table", read(tab, V * E, "table").reshape(V, E), tr.scatter_add_rows(src, ids, table, V))


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
CE_CASES = [(1, 1, 0), (63, 6, 1), (64, 1027, 0), (65, 6, 0), (729, 1027, 0), (729, 6, 1), (1, 6, 1), (64, 1, 1), (65, 1027, 1), (63, 1, 0)]


@pytest.mark.parametrize("V,n,odd", CE_CASES)
def test_cross_entropy_forward(V, n, odd):
    ld = V + 3 if odd else (V + 63) // 64 * 64
    logits, target, gs = tr.ce_inputs(n, V)
    lg = torch.full((n * ld,), 1e30, device=DEV)                       # (pitch columns hold a value that would dominate the row)
    fill_pitched(lg, logits, ld, tr.F32)
    loss, lse, td = nans(n), nans(n), ints(target)
    run(lib().mh_cross_entropy_fwd, lg.data_ptr(), ld, td.data_ptr(), loss.data_ptr(), lse.data_ptr(), n, V)
    ref = tr.ce_fwd(logits, target, V)
    compare("ce_fwd V%d n%d ld%d" % (V, n, ld), "lse", read(lse, n, "lse"), ref["lse"])
    compare("ce_fwd V%d n%d ld%d" % (V, n, ld), "loss", read(loss, n, "loss"), ref["loss"])


@DT
@pytest.mark.parametrize("V,n,odd", CE_CASES)
def test_cross_entropy_backward(V, n, odd, dtype):
    ld = V + 3 if odd else (V + 63) // 64 * 64
    Vpad, ldd = (V + 5, V + 9) if odd else ((V + 8) // 8 * 8, (V + 8) // 8 * 8 + 8)
    logits, target, gs = tr.ce_inputs(n, V)
    lse = tr.ce_fwd(logits, target, V)["lse"][0].astype(np.float32)      # (the reference's lse: the forward kernel cannot mask a backward error)
    lg = torch.full((n * ld,), 1e30, device=DEV)
    fill_pitched(lg, logits, ld, tr.F32)
    td, ld_, gd = ints(target), dev(lse), dev(gs)
    dl = nans(n * ldd, dtype)
    run(lib().mh_cross_entropy_bwd, lg.data_ptr(), ld, td.data_ptr(), ld_.data_ptr(), gd.data_ptr(), dl.data_ptr(), ldd, n, V, Vpad, dtype)
    got = read_pitched(dl, n, Vpad, ldd, "dlogits")
    assert np.all(got[:, V:] == 0), "columns [V, Vpad) must be exactly 0"
    compare("ce_bwd V%d n%d %s" % (V, n, TNAME[dtype]), "dlogits", got[:, :V], tr.ce_bwd(logits, target, lse, gs, V, dtype))


# ------------------------------------------------------------------------------------------------------------------ squared error
def _offset(a, off):
    """device copy of float32 `a`, `off` floats into its allocation"""
    buf = torch.empty(a.size + 4, device=DEV)
    buf[off:off + a.size] = dev(a.reshape(-1))
    return buf, buf.data_ptr() + 4 * off


SQDIFF_MEAN_CASES = [(1, 1, 0, 1.0, 0), (4, 3, 1, 0.37, 0), (7, 3, 1, 1.0, 0), (4096, 1, 0, 0.37, 0), (4099, 3, 1, 0.37, 0), (4096, 3, 1, 1.0, 0), (4096, 3, 1, 0.37, 1),
                     (7, 1, 0, 0.37, 0), (4, 1, 1, 1.0, 1)]


@pytest.mark.parametrize("per_batch,B,with_b,scale_a,off", SQDIFF_MEAN_CASES)
def test_squared_error_mean(per_batch, B, with_b, scale_a, off):
    a, b = tr.sqdiff_inputs(per_batch, B, with_b)
    abuf, ap = _offset(a, off)
    bbuf, bp = _offset(b, 0) if with_b else (None, None)
    out = nans(B)
    keys = tc.keys_of(lambda: run(lib().mh_sqdiff_mean, ap, bp, scale_a, out.data_ptr(), B, per_batch))
    assert keys == ["sqdiff_mean_kernel | vec=%d" % (per_batch % 4 == 0 and not off)], keys
    compare("sqdiff_mean n%d B%d b%d s%g off%d" % (per_batch, B, with_b, scale_a, off), "out", read(out, B, "out"), tr.sqdiff_mean(a, b, scale_a))


@pytest.mark.parametrize("per_batch,B,with_b,scale_a,outs,acc", [(1, 1, 0, 1.0, "a", 0), (4, 3, 1, 0.37, "ab", 0), (7, 3, 1, 1.0, "b", 0), (4096, 1, 1, 0.37, "ab", 1),
                                                               (4099, 3, 0, 0.37, "a", 1), (4099, 3, 1, 1.0, "b", 1), (WRAP // 3, 3, 1, 0.37, "ab", 0),
                                                               (WRAP // 3, 3, 0, 1.0, "a", 1)])
def test_squared_error_backward(per_batch, B, with_b, scale_a, outs, acc):
    assert per_batch < 10000 or B * per_batch == WRAP
    g = tr.rng(per_batch + B + acc)
    a = (g.standard_normal((B, per_batch)) + 0.5).astype(np.float32)
    b = g.standard_normal((B, per_batch)).astype(np.float32) if with_b else None
    gs = (g.standard_normal(B) * 3).astype(np.float32)
    starts = {k: (g.standard_normal((B, per_batch)).astype(np.float32) if acc else None) for k in "ab"}
    ad, bd, gd = dev(a.reshape(-1)), (dev(b.reshape(-1)) if with_b else None), dev(gs)
    bufs = {}
    for k in outs:
        bufs[k] = nans(B * per_batch)
        if acc:
            bufs[k][:B * per_batch] = dev(starts[k].reshape(-1))
    run(lib().mh_sqdiff_bwd, ad.data_ptr(), _lib.ptr(bd), scale_a, gd.data_ptr(), _lib.ptr(bufs.get("a")), _lib.ptr(bufs.get("b")), acc, B, per_batch)
    ref = tr.sqdiff_bwd(a, b, scale_a, gs, starts["a"], starts["b"])
    for k in outs:
        compare("sqdiff_bwd n%d B%d b%d s%g acc%d" % (per_batch, B, with_b, scale_a, acc), "d" + k, read(bufs[k], B * per_batch, "d" + k), ref["d" + k])


@pytest.mark.parametrize("B,per_batch,E,with_mask,with_scale,acc", [(3, 16 * 5, 16, 1, 1, 0), (2, 128 * 3, 128, 0, 1, 1), (3, 128 * 3, 128, 1, 0, 0), (1, 16, 16, 0, 0, 1),
                                                                  (3, 16 * 5, 16, 1, 1, 1), (3, WRAP // 3, 16, 1, 1, 0), (3, WRAP // 3, 128, 1, 1, 1)])
def test_scale_rows(B, per_batch, E, with_mask, with_scale, acc):
    g = tr.rng(per_batch + E + acc)
    total = B * per_batch
    src = g.standard_normal((B, per_batch)).astype(np.float32)
    scale = (g.standard_normal(B) * 2).astype(np.float32) if with_scale else None
    mask = g.integers(0, 2, (total + E - 1) // E).astype(np.int32) if with_mask else None      # (one entry per token: element i reads mask[i / E])
    start = g.standard_normal((B, per_batch)).astype(np.float32) if acc else None
    sd, scd, md = dev(src.reshape(-1)), (dev(scale) if with_scale else None), (ints(mask) if with_mask else None)
    dst = nans(total)
    if acc:
        dst[:total] = dev(start.reshape(-1))
    run(lib().mh_scale_rows, sd.data_ptr(), _lib.ptr(scd), _lib.ptr(md), dst.data_ptr(), acc, B, per_batch, E)
    compare("scale_rows B%d n%d E%d m%d s%d acc%d" % (B, per_batch, E, with_mask, with_scale, acc), "dst", read(dst, total, "dst"),
            tr.scale_rows(src, scale, mask, E, start))


# ------------------------------------------------------------------------------------------------------------------ row softmax
SOFTMAX_CASES = [(1, 1, 1.0), (63, 6, 0.125), (64, 6, 1.0), (65, 1, 0.125), (528, 6, 0.125), (65, 6, 1.0), (528, 1, 1.0)]


@DT
@pytest.mark.parametrize("L,rows,scale", SOFTMAX_CASES)
def test_softmax_rows_forward_and_backward(L, rows, scale, dtype):
    ld = L + (8 if L % 2 == 0 else 3)
    s, dp = tr.softmax_inputs(L, rows, scale, dtype)                       # one row with a dominant score: +60 after scaling
    name = "softmax L%d r%d s%g %s" % (L, rows, scale, TNAME[dtype])
    buf = nans(rows * ld, dtype)
    fill_pitched(buf, s, ld, dtype)
    run(lib().mh_softmax_rows, buf.data_ptr(), rows, L, ld, scale, dtype)
    ref = tr.softmax_rows(s, scale, dtype)
    compare(name, "p", read_pitched(buf, rows, L, ld, "p"), ref)
    # backward on the reference's probabilities as stored, in place on dp
    p = tr.q(ref[0], dtype)
    pbuf, dbuf = nans(rows * ld, dtype), nans(rows * ld, dtype)
    fill_pitched(pbuf, p, ld, dtype)
    fill_pitched(dbuf, dp, ld, dtype)
    run(lib().mh_softmax_bwd_rows, pbuf.data_ptr(), dbuf.data_ptr(), rows, L, ld, scale, dtype)
    compare(name, "ds", read_pitched(dbuf, rows, L, ld, "ds"), tr.softmax_bwd_rows(p, dp, scale, dtype))
    exact(name, "p (input)", read_pitched(pbuf, rows, L, ld, "p"), p)


# ------------------------------------------------------------------------------------------------------------------ activations
ACT_IDS = ["none", "tanh", "gelu", "silu"]
ACT_CASES = [(act, n, dtype) for act in range(4) for n in (1, 255) for dtype in (tr.BF16, tr.F32)] + [
    (tr.ACT_GELU, WRAP, tr.BF16), (tr.ACT_TANH, WRAP, tr.F32), (tr.ACT_SILU, WRAP, tr.F32), (tr.ACT_NONE, WRAP, tr.BF16)]


@pytest.mark.parametrize("act,n,dtype", ACT_CASES, ids=lambda v: None)
def test_activation_forward_and_backward(act, n, dtype):
    x = tr.act_inputs(n, dtype, seed=act + n)
    assert (x == 0).any() and (n == 1 or (x.min() == -12 and x.max() == 12))
    dy = tr.q(tr.rng(n).standard_normal(n) * 2, dtype)
    name = "act %s n%d %s" % (ACT_IDS[act], n, TNAME[dtype])
    xd, dyd, y, dx = dev(x, dtype), dev(dy, dtype), nans(n, dtype), nans(n, dtype)
    run(lib().mh_act_fwd, xd.data_ptr(), y.data_ptr(), n, act, dtype)
    run(lib().mh_act_bwd, dyd.data_ptr(), xd.data_ptr(), dx.data_ptr(), n, act, dtype)
    compare(name, "y", read(y, n, "y"), tr.act_fwd(x, act, dtype))
    compare(name, "dx", read(dx, n, "dx"), tr.act_bwd(dy, x, act, dtype))


# ------------------------------------------------------------------------------------------------------------------ the two adds (exact)
@pytest.mark.parametrize("dtype,B,L,H,pad,kernel", [(tr.BF16, 2, 5, 128, 8, "add_pos_time8_kernel"), (tr.BF16, 3, 5, 520, 0, "add_pos_time8_kernel"),
                                                   (tr.BF16, 2, 5, 12, 8, "add_pos_time_kernel<bf16>"), (tr.F32, 2, 5, 16, 8, "add_pos_time_kernel<float>"),
                                                   (tr.BF16, 2, 5, 128, 4, "add_pos_time_kernel<bf16>"), (tr.BF16, 3, WRAP // 21, 7, 1, "add_pos_time_kernel<bf16>"),
                                                   (tr.F32, 3, WRAP // 21, 7, 0, "add_pos_time_kernel<float>")])
def test_add_pos_time_bit_for_bit(dtype, B, L, H, pad, kernel):
    assert L < 100 or B * L * H == WRAP
    g = tr.rng(L + H)
    ldx = H + pad
    x = tr.q(g.standard_normal((B * L, H)), dtype)
    pos, emb = g.standard_normal((L, H)).astype(np.float32), g.standard_normal((B, H)).astype(np.float32)
    xb = torch.full((B * L * ldx,), 77.0, dtype=TD[dtype], device=DEV)
    fill_pitched(xb, x, ldx, dtype)
    pd, ed, out = dev(pos), dev(emb), nans(B * L * H, dtype)
    keys = tc.keys_of(lambda: run(lib().mh_add_pos_time, xb.data_ptr(), ldx, pd.data_ptr(), ed.data_ptr(), out.data_ptr(), B, L, H, dtype))
    assert keys == [kernel], keys
    exact("add_pos_time", "out", read(out, B * L * H, "out").reshape(B, L, H), tr.add_pos_time(x.reshape(B, L, H), pos, emb, dtype))


@DT
@pytest.mark.parametrize("n", [1, 255, WRAP])
def test_add_inplace_bit_for_bit(n, dtype):
    g = tr.rng(n)
    a, b = tr.q(g.standard_normal(n) * 3, dtype), tr.q(g.standard_normal(n), dtype)
    dst = nans(n, dtype)
    dst[:n] = dev(a, dtype)
    bd = dev(b, dtype)
    run(lib().mh_add_inplace, dst.data_ptr(), bd.data_ptr(), n, dtype)
    exact("add_inplace", "dst", read(dst, n, "dst"), tr.add_inplace(a, b, dtype))
    exact("add_inplace", "src", host(bd), b)


def test_sum_slices_against_float64():
    g = tr.rng(12)
    S, n = 5, 4 * 1031
    x = g.standard_normal((S, n)).astype(np.float32)
    xd, out = dev(x.reshape(-1)), nans(n)
    run(lib().mh_sum_slices, xd.data_ptr(), S, n, out.data_ptr())
    ref, bound = tr.col_sum(x[None])
    compare("sum_slices", "out", read(out, n, "out"), (ref[0], bound[0]))


# ------------------------------------------------------------------------------------------------------------------ layout movers (exact)
def _distinct(n, dtype, seed):
    """values that tell a misplaced element apart (bf16: 2^16 patterns, drawn at random)"""
    return tr.q(tr.rng(seed).standard_normal(n) * 8, dtype)


@pytest.mark.parametrize("dtype,rows,cols,batch,pad_in,pad_out,kernel", [
    (tr.BF16, 128, 64, 3, 8, 8, "transpose64_kernel"), (tr.BF16, 64, 192, 1, 0, 0, "transpose64_kernel"), (tr.BF16, 45, 70, 3, 1, 2, "transpose_kernel<bf16>"),
    (tr.F32, 64, 64, 1, 0, 3, "transpose_kernel<float>"), (tr.BF16, 64, 64, 3, 8, 1, "transpose_kernel<bf16>"), (tr.F32, 33, 31, 3, 5, 0, "transpose_kernel<float>")])
def test_transpose_bit_for_bit(dtype, rows, cols, batch, pad_in, pad_out, kernel):
    ld_in, ld_out = cols + pad_in, rows + pad_out
    s_in, s_out = rows * ld_in + (16 if batch > 1 else 0), cols * ld_out + (24 if batch > 1 else 0)
    flat = _distinct(batch * s_in, dtype, rows + cols)
    xd, out = dev(flat, dtype), nans(batch * s_out, dtype)
    keys = tc.keys_of(lambda: run(lib().mh_transpose, xd.data_ptr(), ld_in, s_in, out.data_ptr(), ld_out, s_out, rows, cols, batch, dtype))
    assert keys == [kernel], keys
    o = read(out, batch * s_out, "out")
    for b in range(batch):
        x = flat[b * s_in:b * s_in + rows * ld_in].reshape(rows, ld_in)[:, :cols]
        blk = o[b * s_out:(b + 1) * s_out]
        body = blk[:cols * ld_out].reshape(cols, ld_out)
        assert np.isnan(body[:, rows:]).all() and np.isnan(blk[cols * ld_out:]).all(), "written into the output's pad"
        exact("transpose b%d" % b, "out", body[:, :rows], x.T)


# (mode, dtype, B, L, nh, dh, kernel)
HP_CASES = [
    (0, tr.BF16, 2, 64, 3, 24, "head_permute8_kernel"), (0, tr.F32, 2, 64, 3, 32, "head_permute_kernel<float>"), (0, tr.BF16, 1, 1024, 2, 128, "head_permute8_kernel"),
    (1, tr.BF16, 1, 1024, 2, 64, "head_permute8_kernel"), (1, tr.F32, 2, 64, 3, 24, "head_permute_kernel<float>"), (1, tr.BF16, 2, 528, 3, 32, "head_permute8_kernel"),
    (2, tr.BF16, 2, 64, 3, 32, "head_transpose_kernel<32>"), (2, tr.BF16, 2, 528, 3, 64, "head_permute_kernel<bf16>"), (2, tr.BF16, 2, 64, 3, 24, "head_permute_kernel<bf16>"),
    (2, tr.F32, 2, 64, 3, 32, "head_permute_kernel<float>"), (2, tr.BF16, 1, 1024, 2, 128, "head_transpose_kernel<128>"),
    (3, tr.BF16, 1, 1024, 3, 64, "head_transpose_kernel<64>"), (3, tr.BF16, 2, 528, 2, 128, "head_permute_kernel<bf16>"), (3, tr.F32, 2, 64, 3, 24, "head_permute_kernel<float>"),
    (3, tr.BF16, 2, 64, 3, 32, "head_transpose_kernel<32>"),
    # the scalar kernel's second sweep: B L nh dh = 16384 x 256 + 257 elements
    (1, tr.F32, 3, WRAP // 21, 1, 7, "head_permute_kernel<float>"), (0, tr.BF16, 3, WRAP // 21, 1, 7, "head_permute_kernel<bf16>"),
    (4, tr.BF16, 2, 64, 3, 128, "head_transpose_kernel<128>"), (4, tr.BF16, 1, 1024, 3, 32, "head_transpose_kernel<32>"), (4, tr.BF16, 3, 64, 2, 64, "head_transpose_kernel<64>"),
]


@pytest.mark.parametrize("mode,dtype,B,L,nh,dh,kernel", HP_CASES)
def test_head_permute_bit_for_bit(mode, dtype, B, L, nh, dh, kernel):
    H = nh * dh
    ld = H + 8
    n = B * L * H
    if mode == 1:      # heads [B, nh, L, dh] -> tokens [B L, ld]
        x = _distinct(n, dtype, L + dh)
        xd, out = dev(x, dtype), nans(B * L * ld, dtype)
        keys = tc.keys_of(lambda: run(lib().mh_head_permute, xd.data_ptr(), out.data_ptr(), ld, B, L, nh, dh, mode, dtype))
        got = read_pitched(out, B * L, H, ld, "tokens")
    else:
        tok = _distinct(B * L * ld, dtype, L + dh + mode).reshape(B * L, ld)      # (the pad columns hold numbers too)
        x = tok[:, :H]
        xd = dev(tok.reshape(-1), dtype)
        slack = 256 if mode == 4 else 0
        out = nans(n + slack, dtype)
        keys = tc.keys_of(lambda: run(lib().mh_head_permute, xd.data_ptr(), out.data_ptr(), ld, B, L, nh, dh, mode, dtype))
        o = read(out, n + slack, "heads")
        assert np.all(o[n:] == 0), "mode 4 zeroes the 256 elements behind the last row"
        got = o[:n]
    assert keys == ["%s | mode=%d" % (kernel, mode)], keys
    exact("head_permute mode %d" % mode, "out", got.reshape(-1), tr.head_permute(x, B, L, nh, dh, mode).reshape(-1))


def test_head_permute_rejects_mode_4_without_its_vector_path():
    t = nans(4096)
    rejected(lib().mh_head_permute, t.data_ptr(), t.data_ptr(), 40, 1, 64, 1, 32, 4, tr.F32)
    rejected(lib().mh_head_permute, t.data_ptr(), t.data_ptr(), 40, 1, 24, 1, 32, 3, tr.BF16)      # modes 3 / 4: seq_len % 16
    assert np.isnan(host(t)).all()


@pytest.mark.parametrize("rows,cols,ld_rm,ld_pan", [(45, 64, 72, 48), (1, 32, 32, 1), (300, 128, 128, 301)])
def test_repack_panel_each_direction(rows, cols, ld_rm, ld_pan):
    x = _distinct(rows * cols, tr.BF16, rows).reshape(rows, cols)
    # row-major -> panels
    rm = torch.full((rows * ld_rm,), 55.0, dtype=torch.bfloat16, device=DEV)
    fill_pitched(rm, x, ld_rm, tr.BF16)
    n_pan = (cols // 32) * ld_pan * 32
    pan = nans(n_pan, tr.BF16)
    run(lib().mh_repack_panel, rm.data_ptr(), ld_rm, pan.data_ptr(), ld_pan, rows, cols, 1)
    got = read(pan, n_pan, "panels").reshape(cols // 32, ld_pan, 32)
    want = tr.to_panel(x, ld_pan)
    assert np.isnan(got[:, rows:]).all(), "written into panel rows behind the last row"
    exact("repack to panels", "out", got[:, :rows], want[:, :rows])
    # panels -> row-major (rows behind the last hold numbers the kernel must not move)
    src = _distinct(n_pan, tr.BF16, rows + 1).reshape(cols // 32, ld_pan, 32)
    src[:, :rows] = want[:, :rows]
    sd, out = dev(src.reshape(-1), tr.BF16), nans(rows * ld_rm, tr.BF16)
    run(lib().mh_repack_panel, sd.data_ptr(), ld_pan, out.data_ptr(), ld_rm, rows, cols, 0)
    exact("repack to rows", "out", read_pitched(out, rows, cols, ld_rm, "rows"), x)


def test_weight_prep_panel_forms():
    """mh_weight_prep with both destinations as K32 panels (pad_ bits 0 and 1: what the panel tape's GEMMs read), against the documented
    layout; tests/test_kernels_gpu.py covers the row-major forms"""
    rows, cols = 128, 192
    W = tr.rng(5).standard_normal((rows, cols)).astype(np.float32)
    ld_dst, ld_t = rows + 3, cols + 5
    n1, n2 = (cols // 32) * ld_dst * 32, (rows // 32) * ld_t * 32
    dst, dst_t, Wd = nans(n1, tr.BF16), nans(n2, tr.BF16), dev(W)
    items = (_lib.WPrepItem * 1)(_lib.WPrepItem(Wd.data_ptr(), dst.data_ptr(), dst_t.data_ptr(), rows, cols, ld_dst, ld_t, 0, 3))
    table = torch.frombuffer(bytearray(C.string_at(C.addressof(items), C.sizeof(items))), dtype=torch.uint8).to(DEV)
    run(lib().mh_weight_prep, table.data_ptr(), 1, (rows // 64) * (cols // 64))
    wb = tr.q(W, tr.BF16)
    for what, buf, n, x, ld in (("dst", dst, n1, wb, ld_dst), ("dst_t", dst_t, n2, np.ascontiguousarray(wb.T), ld_t)):
        got = read(buf, n, what).reshape(-1, ld, 32)
        assert np.isnan(got[:, x.shape[0]:]).all(), "%s: written into panel rows behind the last row" % what
        exact("weight_prep panels", what, got[:, :x.shape[0]], tr.to_panel(x, ld)[:, :x.shape[0]])
