"""Parity matrix of the kernels a sampling step launches outside the GEMMs and attention (csrc/elementwise.hip, csrc/norm.hip,
csrc/rounding.hip, csrc/headtail.hip, the two rounding helpers of csrc/gemm.hip): every C entry point called through the library's ABI
against the references of tests/step_ref.py, EVERY element of EVERY output, at the smallest shapes that reach each path - the scalar
update kernel (E % 4 != 0, a tensor 4 bytes off a 16-byte boundary), per-batch coefficient rows, the three mask forms, the slot fold's
tie / -inf / NaN rules, rows % 4 != 0 and widths with a single lane in the last chunk column for the LayerNorms, every panel
instantiation with pitches wider than the rows, token / vocabulary / embedding sizes on both sides of the 64-wide tiles of the
argmax kernel with duplicated table rows across its lanes and tiles, row blocks of head and tail that span batch items and end in a
partial block, and the second sweep of the grid-stride loops (ew_grid caps a launch at 8192 blocks x 256 threads = 2 097 152 work items).

Rules of every case: every output and scratch buffer starts as NaN (-1 for indices) and is larger than the kernel may write; whatever
lies outside the documented output must be untouched afterwards.  The diffusion arithmetic, the layout movers and the slot fold are
compared bit for bit with numpy float32 / indexing; the others element by element with |got - ref| <= bound (tests/step_ref.py;
tests/test_step_bound_cpu.py holds a float32 restatement to half of each bound); an argbest by the margin rule (step_ref.argbest_check)
with at most 1 % of rows in the near-tie class.  Cases that the census table rests on record their launch (tests/step_census.py) and
assert which kernel and path they ran.

The truncated normal is compared with a host restatement (Philox4x32-10, Box-Muller in float64, the rejection loop).  The device uses the
hardware log / sqrt / sin / cos, so the tolerance is four times the worst |device - restatement| of the bound-0 case (2^20 elements),
which must not exceed 1e-4 (a wrong counter word gives O(1) differences); an element is left out when a candidate the restatement
examined for it lies within the tolerance of +-bound, at most 1 % per case.  Attempts above 255 (the second counter word's top byte) are
not reachable by search - 5e-10 per element at bound 0.1 - and no case is contrived for them.
Measured on an MI355X: see profiles/step_census_and_mutations.txt."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import step_census as sc
import step_ref as sr

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import check, current_stream, lib  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SLACK = 256
CAP = 8192 * 256                      # work items of one sweep of a grid-stride launch
F32, BF16 = sr.F32, sr.BF16
TD = {BF16: torch.bfloat16, F32: torch.float32}
TNAME = {BF16: "bf16", F32: "f32"}
MH_ERR_INVALID, MH_ERR_UNSUPPORTED = -1, -3


# ------------------------------------------------------------------------------------------------------------------ buffers
def dev(a, dtype=F32):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t.to(TD[dtype]) if dtype == BF16 else t


def ints(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def nans(n, dtype=F32):
    return torch.full((int(n) + SLACK,), NAN, dtype=TD[dtype], device=DEV)


def minus(n):
    return torch.full((int(n) + SLACK,), -1, dtype=torch.int32, device=DEV)


def host(t):
    return t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def read(t, n, what):
    """the first n elements of a NaN (-1) initialised buffer; everything behind them must be untouched"""
    a = host(t)
    tail = a[n:]
    assert (np.isnan(tail).all() if t.is_floating_point() else (tail == -1).all()), "%s: written behind its %d elements" % (what, n)
    return a[:n]


def read_pitched(t, rows, cols, ld, what):
    a = host(t)
    body = a[:rows * ld].reshape(rows, ld)
    assert np.isnan(body[:, cols:]).all() and np.isnan(a[rows * ld:]).all(), "%s: written outside its [%d, %d] (pitch %d)" % (what, rows, cols, ld)
    return body[:, :cols]


def read_panel(t, nkb, rows, ld, what):
    """bf16 panels [nkb, ld, 32] out of a NaN buffer -> [rows, 32 nkb]; the rows behind `rows` of every panel and the tail still NaN"""
    a = host(t)
    p = a[:nkb * ld * 32].reshape(nkb, ld, 32)
    assert np.isnan(p[:, rows:]).all() and np.isnan(a[nkb * ld * 32:]).all(), "%s: written outside its %d rows (pitch %d)" % (what, rows, ld)
    return sr.from_panel(p, rows)


def untouched(t, what):
    a = host(t)
    assert (np.isnan(a).all() if t.is_floating_point() else (a == -1).all()), "%s: written by a rejected call" % what


def run(fn, *args):
    check(fn(*args, current_stream()), fn.__name__)


def rejected(fn, *args):
    rc = fn(*args, current_stream())
    assert rc != 0 and lib().mh_last_error()
    return rc


def exact(case, name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    if got.dtype.kind == "f":
        diff = got.astype(np.float32).view(np.uint32) != want.astype(np.float32).view(np.uint32)
    else:
        diff = got != want
    if diff.any():
        i = np.unravel_index(int(np.argmax(diff)), diff.shape)
        pytest.fail("%s %s: %d of %d elements differ, first at %s: got %r want %r" % (case, name, int(diff.sum()), diff.size, i, got[i], want[i]))


def compare(case, name, got, pair):
    ref, bound = pair
    bound = np.broadcast_to(bound, ref.shape)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), "%s %s: %d elements never written (still NaN) or not finite, first at %s" % (
        case, name, int(bad.sum()), np.unravel_index(int(np.argmax(bad)), ref.shape))
    print("STEP-MATRIX %s %s %.3f" % (case, name, sr.ratio(got, ref, bound)))
    err = np.abs(got - ref)
    out = err > bound
    if out.any():
        i = np.unravel_index(int(np.argmax(err - bound)), ref.shape)
        pytest.fail("%s %s: %d of %d elements outside their bound; worst at %s: got %.9g ref %.9g (bound %.3g)"
                    % (case, name, int(out.sum()), out.size, i, got[i], ref[i], bound[i]))


def recorded(fn):
    """fn() under the launch recorder -> the census keys it launched"""
    return sc.keys_of(fn)


def mask_of(form, B, L, E, seed):
    g = sr.rng(seed)
    if form == "none":
        return None
    m = (g.uniform(size=(B, L) if form == "row" else (B, L, E)) < 0.6).astype(np.int32)
    m.reshape(-1)[:2] = (0, 1)
    return m


# ------------------------------------------------------------------------------------------------------------------ 1. q_sample
Q_CASES = [(3, 5, 6, "none"), (3, 5, 6, "row"), (3, 5, 6, "elem"), (2, 8200, 128, "row")]


@pytest.mark.parametrize("B,L,E,form", Q_CASES)
def test_q_sample_bit_for_bit(B, L, E, form):
    assert (B * L * E > CAP) == (L == 8200)
    g = sr.rng(B * L + E)
    x0, nz = g.standard_normal((B, L, E)).astype(np.float32), g.standard_normal((B, L, E)).astype(np.float32)
    a, s = g.uniform(0.1, 1, B).astype(np.float32), g.uniform(0.1, 1, B).astype(np.float32)
    m = mask_of(form, B, L, E, 3)
    out = nans(B * L * E)
    md = ints(m) if m is not None else None
    x0d, nzd, ad, sd = dev(x0), dev(nz), dev(a), dev(s)
    keys = recorded(lambda: run(lib().mh_q_sample, x0d.data_ptr(), nzd.data_ptr(), ad.data_ptr(), sd.data_ptr(), _lib.ptr(md), int(form == "elem"),
                                out.data_ptr(), B, L * E, E))
    assert keys == ["q_sample_kernel"]
    exact("q_sample %s" % form, "out", read(out, B * L * E, "out").reshape(B, L, E), sr.q_sample(x0, nz, a, s, m))


# ------------------------------------------------------------------------------------------------------------------ 2. update kernels
# (kind, form, x0 source, clip, mask, coef_per_batch, noise, pred, mean); form: "vec" E = 8 aligned | "e6" E = 6 | "off" E = 8, x_t 4 bytes off
_OPTS = [("model", 0, "none", 0, 0, 0, 0), ("idx", 1, "row", 1, 1, 1, 1), ("model", 1, "elem", 1, 1, 1, 0), ("idx", 0, "elem", 0, 0, 1, 1),
         ("idx", 1, "row", 0, 1, 1, 0)]          # (the last: the form the loops launch without the fused rounding)
EPI_CASES = [(kind, form) + o for kind in ("p", "ddim") for form in ("vec", "e6", "off") for o in _OPTS]
EPI_BIG = ("p", "vec", "model", 1, "row", 1, 1, 1, 0)


def _epi_id(c):
    return "%s-%s-x0%s-clip%d-mask%s-cpb%d-noise%d-pred%d-mean%d" % c


def epi_case_key(c):
    kind, form, x0s, clip, form_m, cpb, noise, pred, mean = c
    name = "step_epilogue%s_kernel<%s>" % ("4" if form == "vec" else "", "true" if kind == "ddim" else "false")
    return sc.epilogue_key(name, x0s, form_m, cpb, "given" if noise else "none")


def _epi_inputs(c, B, L, E, V=11):
    kind, form, x0s, clip, form_m, cpb, noise, pred, mean = c
    g = sr.rng(zlib.crc32(_epi_id(c).encode()) % 1000 + B)
    tab = sr.coef_table(kind, 0.5 if kind == "ddim" else 0.0)
    ts = [0, 1999, 1000][:B] if B <= 3 else list(g.integers(0, 2000, B))
    coef = tab[ts] if cpb else tab[[1999 if clip else 1000]]       # (sigma > 0 in every single-row case; t = 0 is among the per-batch rows)
    table = (1.5 * g.standard_normal((V, E))).astype(np.float32)
    idx = g.integers(0, V, (B, L)).astype(np.int32)
    model = (1.5 * g.standard_normal((B, L, E))).astype(np.float32)
    xt, nz, xs = (g.standard_normal((B, L, E)).astype(np.float32) for _ in range(3))
    m = mask_of(form_m, B, L, E, 5)
    x0 = table[idx] if x0s == "idx" else model
    ref = sr.step_update(x0, xt, nz if noise else None, coef, clip, kind == "ddim", m, xs)
    return dict(coef=coef, table=table, idx=idx, model=model, xt=xt, nz=nz, xs=xs, mask=m, ref=ref)


def _run_epilogue(c, B, L, E, d, offset_xt):
    kind, form, x0s, clip, form_m, cpb, noise, pred, mean = c
    n = B * L * E
    out, predb, meanb = nans(n), nans(n), nans(n)
    xt_buf = torch.zeros(n + 8, device=DEV)
    xt_d = xt_buf[1:n + 1] if offset_xt else xt_buf[:n]
    xt_d.copy_(dev(d["xt"]).view(-1))
    assert (xt_d.data_ptr() % 16 == 4) == bool(offset_xt)
    keep = [dev(d["model"]), dev(d["nz"]), ints(d["idx"]), dev(d["table"]), dev(d["coef"]), ints(d["mask"]) if d["mask"] is not None else None, dev(d["xs"])]
    model_d, nz_d, idx_d, table_d, coef_d, mask_d, xs_d = keep
    P = _lib.ptr
    args = [P(model_d) if x0s == "model" else None, P(xt_d), P(nz_d) if noise else None, P(idx_d) if x0s == "idx" else None,
            P(table_d) if x0s == "idx" else None, P(coef_d), cpb, clip, P(mask_d), int(form_m == "elem"), P(xs_d) if mask_d is not None else None,
            P(out), P(predb) if pred else None]
    if kind == "p":
        keys = recorded(lambda: run(lib().mh_p_sample_epilogue, *args, P(meanb) if mean else None, B, L * E, E))
    else:
        keys = recorded(lambda: run(lib().mh_ddim_epilogue, *args, B, L * E, E))
    got = [read(out, n, "out").reshape(B, L, E), read(predb, n if pred else 0, "pred"), read(meanb, n if (mean and kind == "p") else 0, "mean")]
    return keys, got


def _check_epilogue(name, c, got, ref, B, L, E):
    kind, pred, mean = c[0], c[7], c[8]
    exact(name, "sample", got[0], ref[0])
    if pred:
        exact(name, "pred_xstart", got[1].reshape(B, L, E), ref[1])
    if mean and kind == "p":
        exact(name, "mean", got[2].reshape(B, L, E), ref[2])


@pytest.mark.parametrize("case", EPI_CASES, ids=_epi_id)
def test_update_kernels_bit_for_bit(case):
    form = case[1]
    B, L, E = 3, 5, 6 if form == "e6" else 8
    d = _epi_inputs(case, B, L, E)
    keys, got = _run_epilogue(case, B, L, E, d, offset_xt=form == "off")
    assert keys == [epi_case_key(case)], keys
    _check_epilogue(_epi_id(case), case, got, d["ref"], B, L, E)


@pytest.mark.parametrize("kind", ["p", "ddim"])
def test_update_kernel_forms_agree_bit_for_bit(kind):
    """the 4-wide and the scalar kernel on the same data (the scalar one reached by moving x_t 4 bytes off its boundary)"""
    case = (kind, "vec", "idx", 1, "elem", 1, 1, 1, 1)
    B, L, E = 3, 5, 8
    d = _epi_inputs(case, B, L, E)
    k4, g4 = _run_epilogue(case, B, L, E, d, False)
    k1, g1 = _run_epilogue(case, B, L, E, d, True)
    assert "epilogue4" in k4[0] and "epilogue_kernel" in k1[0]
    for a, b, name in zip(g4, g1, ("sample", "pred", "mean")):
        exact("forms %s" % kind, name, a, b)


def test_update_kernel_second_sweep():
    B, L, E = 66, 1024, 128
    assert B * L * E // 4 > CAP
    d = _epi_inputs(EPI_BIG, B, L, E)
    keys, got = _run_epilogue(EPI_BIG, B, L, E, d, False)
    assert keys == [epi_case_key(EPI_BIG)]
    _check_epilogue("second sweep", EPI_BIG, got, d["ref"], B, L, E)


# ------------------------------------------------------------------------------------------------------------------ 3 / 4. slot fold, in-kernel noise
NSLOTS_V = 12                         # mh_round_slots(729)
# (ddim, nslots, round_idx_out, noise: "none" | "given" | "rng", mask, coef_per_batch, clip)
SLOT_CASES = [(0, 0, 0, "given", "row", 0, 1), (0, 1, 1, "none", "none", 1, 0), (0, NSLOTS_V, 1, "given", "elem", 1, 1), (1, NSLOTS_V, 0, "given", "row", 0, 1),
              (1, 0, 1, "none", "elem", 1, 0), (0, NSLOTS_V, 1, "rng", "row", 0, 1), (1, NSLOTS_V, 1, "rng", "none", 1, 1), (0, 0, 0, "rng", "elem", 0, 1), (0, 0, 1, "rng", "row", 0, 1),
              (1, 0, 0, "rng", "row", 0, 1)]


def _slot_id(c):
    return "%s-ns%d-idxout%d-noise_%s-mask%s-cpb%d-clip%d" % (("ddim" if c[0] else "p",) + c[1:])


def slot_case_key(c):
    ddim, ns, idx_out, noise, form_m, cpb, clip = c
    name = "step_epilogue4_kernel<%s, true%s>" % ("true" if ddim else "false", ", true" if noise == "rng" else "")
    return sc.epilogue_key(name, "slots", form_m, cpb, noise, fold=ns != 0)


def test_slot_count_of_the_vocabulary():
    assert lib().mh_round_slots(729) == NSLOTS_V


def slot_partials(rows, ns, V, seed):
    """partial (score, index) pairs with, in turn: a tie across slots whose smaller index sits in the later slot, all scores -inf (the
    smaller index still wins), all -inf with the GEMM's empty-slot index, a NaN score beside finite ones, all NaN"""
    g = sr.rng(seed)
    pb = (-g.uniform(0, 50, (rows, ns))).astype(np.float32)
    pi = g.integers(0, V, (rows, ns)).astype(np.int32)
    if ns >= 2:
        pb[0, :] = -9.0
        pb[0, [2 % ns, ns - 1]] = -1.25
        pi[0, 2 % ns], pi[0, ns - 1] = 700, 3
        pb[1, :] = -np.inf
        pb[2, :], pi[2, :] = -np.inf, sr.INT_MAX
        pb[3, 0] = np.nan
        pb[4, :] = np.nan
        pb[5, ns // 2] = np.nan
        pb[5, ns - 1] = 0.0
    return pb, pi


def _slots_call(c, B, L, E, V, d, pb, pi, rng_desc, counter):
    ddim, ns, idx_out, noise, form_m, cpb, clip = c
    n, rows = B * L * E, B * L
    out, predb, meanb, ridx = nans(n), nans(n), nans(n), minus(rows)
    keep = [dev(d["xt"]), dev(d["nz"]), dev(pb) if ns else None, ints(pi), dev(d["table"]), dev(d["coef"]),
            ints(d["mask"]) if d["mask"] is not None else None, dev(d["xs"])]
    xt_d, nz_d, pb_d, pi_d, table_d, coef_d, mask_d, xs_d = keep
    P = _lib.ptr
    r = None
    if noise == "rng":
        r = _lib.StepRng()
        r.seed, r.stream_id, r.bound, r.step_counter, r.first_elem = rng_desc["seed"], rng_desc["stream"], rng_desc["bound"], counter.data_ptr(), rng_desc["first"]
    keys = recorded(lambda: run(lib().mh_step_epilogue_slots, ddim, P(xt_d), P(nz_d) if noise == "given" else None, P(pb_d), P(pi_d), ns, P(table_d),
                                P(coef_d), cpb, clip, P(mask_d), int(form_m == "elem"), P(xs_d) if mask_d is not None else None, P(out), P(predb),
                                None if ddim else P(meanb), P(ridx) if idx_out else None, C.byref(r) if r is not None else None, B, L * E, E))
    return keys, (read(out, n, "out").reshape(B, L, E), read(predb, n, "pred").reshape(B, L, E), read(meanb, 0 if ddim else n, "mean"),
                  read(ridx, rows if idx_out else 0, "round_idx_out"))


RNG_DESC = dict(seed=0x1234567887654321, stream=5, bound=1.0, first=4096)
RNG_STEP = 37


@pytest.mark.parametrize("case", SLOT_CASES, ids=_slot_id)
def test_update_with_slot_fold_bit_for_bit(case):
    """mh_step_epilogue_slots: the fold against numpy's, the update against the numpy float32 reference on the folded rows; with an
    mh_step_rng descriptor (first_elem, *step_counter and stream_id all non-zero) against the same call given the noise
    mh_trunc_normal_at writes for that descriptor"""
    ddim, ns, idx_out, noise, form_m, cpb, clip = case
    B, L, E, V = 3, 5, 8, 729
    rows = B * L
    base = ("ddim" if ddim else "p", "vec", "idx", clip, form_m, cpb, int(noise != "none"), 1, 1)
    d = _epi_inputs(base, B, L, E, V)
    pb, pi = slot_partials(rows, max(ns, 1), V, 7 + ns)
    folded = sr.fold_slots(pb, pi) if ns else pi[:, 0].copy()
    if ns == 0:
        pb, pi = None, pi[:, :1]
        assert folded.max() < V
    counter = torch.tensor([RNG_STEP], dtype=torch.int32, device=DEV)
    if noise == "rng":
        nzb = nans(B * L * E + 4)
        nz_d = nzb[:B * L * E]
        run(lib().mh_trunc_normal_at, nzb.data_ptr(), B * L * E, RNG_DESC["first"], RNG_DESC["bound"], RNG_DESC["seed"], RNG_DESC["stream"], counter.data_ptr())
        d["nz"] = host(nz_d).reshape(B, L, E)
        assert np.isfinite(d["nz"]).all() and np.abs(d["nz"]).max() <= 1.0 and d["nz"].std() > 0.3
    keys, got = _slots_call(case, B, L, E, V, d, pb, pi, RNG_DESC, counter)
    assert keys == [slot_case_key(case)], keys
    ref = sr.step_update(d["table"][folded.reshape(B, L)], d["xt"], d["nz"] if noise != "none" else None, d["coef"], clip, bool(ddim), d["mask"], d["xs"])
    name = _slot_id(case)
    if idx_out:
        exact(name, "round_idx_out", got[3], folded)
    exact(name, "sample", got[0], ref[0])
    exact(name, "pred_xstart", got[1], ref[1])
    if not ddim:
        exact(name, "mean", got[2].reshape(B, L, E), ref[2])
    if noise == "rng":
        # the same call given the generator's own output as `noise`
        given = case[:3] + ("given",) + case[4:]
        _, got2 = _slots_call(given, B, L, E, V, d, pb, pi, None, counter)
        for a, b, what in zip(got, got2, ("sample", "pred", "mean", "idx")):
            exact(name + " vs noise from mh_trunc_normal_at", what, a, b)


def test_slots_error_paths_write_nothing():
    B, L, E, V = 1, 2, 8, 16
    out = nans(B * L * E)
    xt, table, coef, pi = dev(np.zeros((B, L, E))), dev(np.zeros((V, E))), dev(sr.coef_table("p")[[5]]), ints(np.zeros(B * L))
    r = _lib.StepRng()
    r.seed, r.stream_id, r.bound, r.step_counter, r.first_elem = 1, 0, 0.0, None, 6        # first_elem % 4 != 0
    rejected(lib().mh_step_epilogue_slots, 0, xt.data_ptr(), None, None, pi.data_ptr(), 0, table.data_ptr(), coef.data_ptr(), 0, 1, None, 0, None,
             out.data_ptr(), None, None, None, C.byref(r), B, L * E, E)
    rejected(lib().mh_step_epilogue_slots, 0, xt.data_ptr() + 4, None, None, pi.data_ptr(), 0, table.data_ptr(), coef.data_ptr(), 0, 1, None, 0, None,
             out.data_ptr(), None, None, None, None, B, L * E, E)                          # a tensor off its 16-byte boundary
    untouched(out, "out")


# ------------------------------------------------------------------------------------------------------------------ 5 / C. truncated normal
def _draw(n, first, bound, seed, stream, step, pad=8):
    buf = nans(n + pad)
    assert buf.data_ptr() % 16 == 0
    counter = torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device=DEV) if step is not None else None
    run(lib().mh_trunc_normal_at, buf.data_ptr(), n, first, bound, seed, stream, _lib.ptr(counter))
    a = host(buf)
    assert np.isnan(a[n:]).all(), "trunc_normal: written behind its %d elements" % n
    return a[:n]


def test_trunc_normal_layout():
    """n = 4099 (a last group of 3) into a 16-byte aligned buffer of n + 8; the draw with first = 8 equals elements 8 onward of the draw
    with first = 0; first % 4 != 0 is rejected and writes nothing"""
    n = 4099
    a = _draw(n, 0, 1.0, 77, 2, 9)
    b = _draw(n - 8, 8, 1.0, 77, 2, 9)
    exact("trunc_normal", "first=8 against [8:] of first=0", b, a[8:])
    assert np.abs(a).max() <= 1.0 and a.std() > 0.3
    buf = nans(16)
    rejected(lib().mh_trunc_normal_at, buf.data_ptr(), 16, 6, 1.0, 77, 2, None)
    rejected(lib().mh_trunc_normal_at, buf.data_ptr() + 4, 8, 0, 1.0, 77, 2, None)
    untouched(buf, "trunc_normal")


TN_CAP = 1e-4
# (bound, n, first, seed, stream, step)
TN_CASES = [(0.0, 1 << 20, 0, 105, 0, None), (1.0, 1 << 16, 1 << 20, 0xDEADBEEF12345, 3, 41), (0.1, 4096, 4096, 9, 200, 2 ** 31 + 5)]


@functools.lru_cache(maxsize=None)
def _tn_tolerance():
    """four times the worst |device - restatement| of the bound-0 case; must not exceed TN_CAP"""
    bound, n, first, seed, stream, step = TN_CASES[0]
    got = _draw(n, first, bound, seed, stream, step)
    ref, _, attempts = sr.trunc_normal(n, first, bound, seed, stream, step or 0)
    assert attempts == 1
    worst = float(np.abs(got - ref).max())
    print("STEP-MATRIX trunc_normal bound 0: worst |device - restatement| %.3e over %d elements" % (worst, n))
    return worst


@pytest.mark.parametrize("case", TN_CASES, ids=lambda c: "bound%g-n%d" % (c[0], c[1]))
def test_trunc_normal_against_host_restatement(case):
    """Measured on an MI355X: worst |device - restatement| 6.7e-07 in the bound-0 case over 2^20 elements (tolerance 2.7e-06, cap 1e-4);
    with it 2.4e-07 at bound 1.0 and 6.1e-08 at bound 0.1, no element excluded."""
    bound, n, first, seed, stream, step = case
    worst = _tn_tolerance()
    tol = 4 * worst
    assert 0 < tol <= TN_CAP, "tolerance %.3g from the bound-0 case exceeds the cap %.3g" % (tol, TN_CAP)
    got = _draw(n, first, bound, seed, stream, step)
    ref, near, attempts = sr.trunc_normal(n, first, bound, seed, stream, step or 0, tol)
    assert near.mean() <= 0.01, "%.4f of the elements lie within the tolerance of the bound" % near.mean()
    err = np.abs(got - ref)[~near]
    print("STEP-MATRIX trunc_normal bound %g: %d attempts, %d of %d elements excluded, worst %.3e (tolerance %.3e)" % (bound, attempts, int(near.sum()), n,
                                                                                                                    float(err.max()), tol))
    assert err.max() <= tol, "%d elements differ by more than %.3g, first at %d" % (int((err > tol).sum()), tol, int(np.argmax(np.abs(got - ref) * ~near > tol)))
    if bound > 0:
        assert np.abs(got).max() <= bound


# ------------------------------------------------------------------------------------------------------------------ 6. loop state
@pytest.mark.parametrize("B", [1, 256, 300])
@pytest.mark.parametrize("pos", [0, 3, 4, 7])
def test_loop_state_kernels(B, pos):
    """mh_step_begin + mh_step_end against mh_step_advance: pos below, at the last step, at and past n_steps (the read is clamped to the
    last step, pos still counts); B past the block size runs the strided emb_row loop a second time"""
    n_steps, T = 4, 2000
    steps = np.array([1999, 1000, 17, 0], dtype=np.int32)
    tab = sr.coef_table("p")
    tab_d, steps_d = dev(tab), ints(steps)
    t = int(steps[min(pos, n_steps - 1)])
    res = []
    for form in ("begin+end", "advance"):
        state = torch.tensor([pos, n_steps, -7, 555], dtype=torch.int32, device=DEV)
        coef, emb = nans(8), minus(B)
        if form == "advance":
            keys = recorded(lambda: run(lib().mh_step_advance, state.data_ptr(), steps_d.data_ptr(), tab_d.data_ptr(), coef.data_ptr(), emb.data_ptr(), B))
            assert keys == ["step_advance_kernel"]
        else:
            keys = recorded(lambda: (run(lib().mh_step_begin, state.data_ptr(), steps_d.data_ptr(), tab_d.data_ptr(), coef.data_ptr(), emb.data_ptr(), B),
                                     run(lib().mh_step_end, state.data_ptr())))
            assert keys == ["step_begin_kernel", "step_end_kernel"]
        st = state.cpu().tolist()
        assert st == [pos + 1, n_steps, t, pos if form == "advance" else 555], (form, st)
        exact(form, "cur_coef", read(coef, 8, "cur_coef"), tab[t])
        exact(form, "emb_row", read(emb, B, "emb_row"), np.full(B, t, dtype=np.int32))
        res.append(st[:3])
    assert res[0] == res[1]


# ------------------------------------------------------------------------------------------------------------------ 7. casts and panels
MOVE_CASES = [(5, 37, 40, 7, 64, 9), (1030, 2040, 2048, 1032, 2048, 1031)]      # rows, cols, ld, rows_out, cols_pad, ld_rows


@pytest.mark.parametrize("rows,cols,ld,rows_out,cols_pad,ld_rows", MOVE_CASES)
def test_casts_and_panel_movers_bit_for_bit(rows, cols, ld, rows_out, cols_pad, ld_rows):
    big = rows > 1000
    assert (rows * cols > CAP) == big
    g = sr.rng(rows + cols)
    src = (3 * g.standard_normal((rows, ld))).astype(np.float32)           # (pitch columns hold numbers too)
    src_d = dev(src)
    a = src[:, :cols]
    for dtype in (F32, BF16):
        # cast_pad: [rows_out, ld] whole, zero outside rows x cols
        out = nans(rows_out * ld, dtype)
        keys = recorded(lambda: run(lib().mh_cast_pad, src_d.data_ptr(), ld, out.data_ptr(), ld, rows, cols, rows_out, dtype))
        assert keys == ["cast_pad_kernel<%s>" % ("bf16" if dtype == BF16 else "float")]
        want = np.zeros((rows_out, ld), dtype=np.float32)
        want[:rows, :cols] = sr.q(a, dtype)
        exact("cast_pad %s" % TNAME[dtype], "out", read(out, rows_out * ld, "cast_pad").reshape(rows_out, ld), want)
        # cast_to_f32: pitched in, pitched out
        stored = dev(sr.q(src, dtype), dtype)
        out = nans(rows * (cols + 3))
        keys = recorded(lambda: run(lib().mh_cast_to_f32, stored.data_ptr(), ld, out.data_ptr(), cols + 3, rows, cols, dtype))
        assert keys == ["cast_to_f32_kernel<%s>" % ("bf16" if dtype == BF16 else "float")]
        exact("cast_to_f32 %s" % TNAME[dtype], "out", read_pitched(out, rows, cols, cols + 3, "cast_to_f32"), sr.q(a, dtype))
    pan = nans((cols_pad // 32) * ld_rows * 32, BF16)
    keys = recorded(lambda: run(lib().mh_pack_panel, src_d.data_ptr(), ld, pan.data_ptr(), ld_rows, rows, cols, cols_pad))
    assert keys == ["pack_panel_kernel"]
    want = sr.pack_panel(a, ld_rows, cols_pad)
    exact("pack_panel", "out", read(pan, want.size, "pack_panel").reshape(want.shape), want)
    back = nans(rows * (cols + 5))
    keys = recorded(lambda: run(lib().mh_unpack_panel_f32, pan.data_ptr(), ld_rows, back.data_ptr(), cols + 5, rows, cols))
    assert keys == ["unpack_panel_kernel"]
    exact("unpack_panel", "out", read_pitched(back, rows, cols, cols + 5, "unpack_panel"), sr.bf16_round(a))


# ------------------------------------------------------------------------------------------------------------------ 8. gather
@pytest.mark.parametrize("n,E,V", [(37, 6, 11), (300, 1, 5), (16400, 128, 729)])
def test_embed_gather_bit_for_bit(n, E, V):
    """ids below 0 and at or above V are clamped to the first / last row (documented); E = 1; one case past the grid cap"""
    assert (n * E > CAP) == (n == 16400)
    g = sr.rng(n + E)
    table = g.standard_normal((V, E)).astype(np.float32)
    ids = g.integers(0, V, n).astype(np.int32)
    ids[:6] = (-1, V, V + 5, -2 ** 31, 2 ** 31 - 1, V - 1)
    out = nans(n * E)
    td, idd = dev(table), ints(ids)
    keys = recorded(lambda: run(lib().mh_embed_gather, td.data_ptr(), idd.data_ptr(), out.data_ptr(), n, E, V))
    assert keys == ["embed_gather_kernel"]
    exact("embed_gather", "out", read(out, n * E, "out").reshape(n, E), table[np.clip(ids.astype(np.int64), 0, V - 1)])


@pytest.mark.parametrize("n,V,ld,ldo", [(5, 37, 40, 41), (2900, 729, 736, 729)])
def test_distance_scores_bit_for_bit(n, V, ld, ldo):
    """-sqrt(clamp((|W_v|^2 + |x_n|^2) - 2 x.W_v, 0)) from a given product: three rounded statements and a correctly rounded square root
    (the argmax of these scores, vocab_argmax_kernel<2>, is covered by tests/test_distance_matrix_gpu.py)"""
    assert (n * V > CAP) == (n == 2900)
    g = sr.rng(n + V)
    dots = g.standard_normal((n, ld)).astype(np.float32)
    wn, xn = g.uniform(0, 3, V).astype(np.float32), g.uniform(0, 3, n).astype(np.float32)
    dots[0, :3] = 50.0                                                   # (a negative distance: clamped)
    out = nans(n * ldo)
    dd, wd, xd = dev(dots), dev(wn), dev(xn)
    keys = recorded(lambda: run(lib().mh_distance_scores, dd.data_ptr(), ld, wd.data_ptr(), xd.data_ptr(), out.data_ptr(), ldo, n, V))
    assert keys == ["distance_scores_kernel"]
    dist = (wn[None] + xn[:, None]) - np.float32(2.0) * dots[:, :V]
    want = -np.sqrt(np.maximum(dist, np.float32(0.0)))
    got = read_pitched(out, n, V, ldo, "out") if ldo > V else read(out, n * V, "out").reshape(n, V)
    exact("distance_scores", "out", got, want)


# ------------------------------------------------------------------------------------------------------------------ 9. split table
@pytest.mark.parametrize("V", [641, 729, 768])
def test_round_split_table(V):
    E, Vp = 128, 768
    g = sr.rng(V)
    table = g.standard_normal((V, E)).astype(np.float32)
    nbytes = int(lib().mh_round_split_bytes(E, V))
    nparts = 3 * (E // 32) * Vp * 32
    assert nbytes == nparts * 2 + Vp * 4
    td = dev(table)
    want = sr.split_table(table, V, E, Vp)
    sq = sr.row_sqnorm(table)
    for given in (False, True):
        buf = torch.full((nbytes + 1024,), 0xFF, dtype=torch.uint8, device=DEV)            # (0xFFFF is a bf16 NaN, 0xFFFFFFFF a float32 one)
        norm = (g.uniform(1, 2, V)).astype(np.float32)
        nd = dev(norm)
        keys = recorded(lambda: run(lib().mh_round_split_table, td.data_ptr(), nd.data_ptr() if given else None, V, E, buf.data_ptr()))
        assert keys == ["round_split_kernel"]
        raw = buf.cpu()
        assert bool((raw[nbytes:] == 0xFF).all()), "round_split_table: written behind its buffer"
        parts = raw[:nparts * 2].view(torch.bfloat16).float().numpy().reshape(want.shape)
        exact("round_split_table V=%d" % V, "hi | hi | lo", parts, want)
        tn = raw[nparts * 2:nbytes].view(torch.float32).numpy()
        assert np.isposinf(tn[V:]).all(), "tnorm beyond V must be +inf"
        if given:
            exact("round_split_table V=%d" % V, "tnorm (the caller's)", tn[:V], norm)
        else:
            compare("round_split_table V=%d" % V, "tnorm", tn[:V], sq)


# ------------------------------------------------------------------------------------------------------------------ 10. row norms
SQNORM_CASES = [(V, E) for V in (1, 5, 729) for E in (1, 63, 64, 65, 128)]


def sqnorm_inputs(V, E):
    return (sr.rng(V * 131 + E).standard_normal((V, E)) * 2).astype(np.float32)


@pytest.mark.parametrize("V,E", SQNORM_CASES)
def test_row_sqnorm(V, E):
    table = sqnorm_inputs(V, E)
    out, td = nans(V), dev(table)
    keys = recorded(lambda: run(lib().mh_row_sqnorm, td.data_ptr(), out.data_ptr(), V, E))
    assert keys == ["row_sqnorm_kernel"]
    compare("row_sqnorm V=%d E=%d" % (V, E), "out", read(out, V, "out"), sr.row_sqnorm(table))


# ------------------------------------------------------------------------------------------------------------------ 11. timestep embedding
TE_CASES = [(dim, dtype) for dim in (32, 33, 128) for dtype in (F32, BF16)]
TE_T = np.array([0.0, 0.5, 17.0, 500.25, 999.5], dtype=np.float32)         # (rescaled timesteps: at most 1999 x 1000 / 2000)


@pytest.mark.parametrize("dim,dtype", TE_CASES, ids=lambda v: str(v))
def test_timestep_embedding(dim, dtype):
    B, ld = len(TE_T), dim + 9
    out, td = nans(B * ld, dtype), dev(TE_T)
    keys = recorded(lambda: run(lib().mh_timestep_embedding, td.data_ptr(), out.data_ptr(), B, dim, ld, 10000.0, dtype))
    assert keys == ["timestep_embedding_kernel<%s>" % ("bf16" if dtype == BF16 else "float")]
    got = read(out, B * ld, "out").reshape(B, ld)
    half = dim // 2
    assert (got[:, 2 * half:] == 0).all(), "the columns behind 2 (dim / 2) are written as zeros"
    compare("timestep_embedding dim=%d %s" % (dim, TNAME[dtype]), "out", got[:, :2 * half], sr.timestep_embedding(TE_T, dim, dtype))


# ------------------------------------------------------------------------------------------------------------------ 12. LayerNorm, row-major
LN_H = (8, 64, 520, 768, 2048)
LN_ROWS = (1, 5, 50)
# (H, dtype, cancel)
LN_CASES = [(H, dtype, 0) for H in LN_H for dtype in (F32, BF16)] + [(768, F32, 1), (768, BF16, 1), (2048, F32, 1)]
# (H, x type, out type, emb_row given, cancel); x: bf16 rows at pitch H + 8 or float32 rows at pitch H + 8
LN_ADD_CASES = [(8, BF16, BF16, 1, 0), (64, F32, BF16, 0, 0), (520, F32, F32, 1, 0), (768, BF16, BF16, 0, 0), (768, F32, BF16, 1, 1), (2048, F32, F32, 0, 0),
                (2048, BF16, BF16, 1, 0)]
LN_ADD_BL = ((1, 1), (5, 1), (1, 3), (2, 3), (17, 3))        # rows 1, 5, 3, 6, 51: L = 3 puts two batch items into one block's four rows
EPS = 1e-12


def _ln_id(c):
    return "H%d-%s%s" % (c[0], TNAME[c[1]], "-mean100" if c[2] else "")


def ln_case_key(c):
    return sc.ln_key("ln_kernel<T, false>", TNAME[c[1]], TNAME[c[1]], 0)


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm_rows(case):
    H, dtype, cancel = case
    for rows in LN_ROWS:
        x, gamma, beta = sr.ln_inputs(rows, H, dtype, H * 3 + rows, cancel)
        out, xd, gd, bd = nans(rows * H, dtype), dev(x, dtype), dev(gamma), dev(beta)
        keys = recorded(lambda: run(lib().mh_layernorm, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, H, EPS, dtype))
        assert keys == [ln_case_key(case)], keys
        compare("layernorm %s rows=%d" % (_ln_id(case), rows), "out", read(out, rows * H, "out").reshape(rows, H),
                sr.layernorm(x, gamma, beta, EPS, dtype, sr.ln_depth(H)))


def _ln_add_id(c):
    return "H%d-x%s-out%s-embrow%d%s" % (c[0], TNAME[c[1]], TNAME[c[2]], c[3], "-mean100" if c[4] else "")


def ln_add_case_key(c):
    return sc.ln_key("ln_kernel<T, true>", TNAME[c[1]], TNAME[c[2]], 1)


def ln_add_inputs(B, L, H, xt, rows_given, cancel, seed):
    x, gamma, beta = sr.ln_inputs(B * L, H, xt, seed, cancel)
    pos, emb_t, rows_of = sr.pos_time_inputs(B, L, H, seed + 1, rows_given)
    if cancel:
        pos, emb_t = pos * np.float32(0.01), emb_t * np.float32(0.01)
    return x, gamma, beta, pos, emb_t, rows_of


@pytest.mark.parametrize("case", LN_ADD_CASES, ids=_ln_add_id)
def test_add_pos_time_layernorm_rows(case):
    H, xt, ot, rows_given, cancel = case
    ld = H + 8
    for B, L in LN_ADD_BL:
        rows = B * L
        x, gamma, beta, pos, emb_t, rows_of = ln_add_inputs(B, L, H, xt, rows_given, cancel, H + rows)
        xbuf = torch.full((rows * ld + 8,), NAN, dtype=TD[xt], device=DEV)
        xbuf[:rows * ld].view(rows, ld)[:, :H] = dev(x, xt)
        out = nans(rows * H, ot)
        keep = [dev(pos), dev(emb_t), ints(rows_of) if rows_given else None, dev(gamma), dev(beta)]
        pd, ed, rd, gd, bd = keep
        keys = recorded(lambda: run(lib().mh_add_pos_time_layernorm, xbuf.data_ptr(), ld, int(xt == F32), pd.data_ptr(), ed.data_ptr(), _lib.ptr(rd),
                                    gd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, L, H, EPS, ot))
        assert keys == [ln_add_case_key(case)], keys
        v = sr.add_pos_time(x, pos, emb_t, rows_of, L)
        compare("add_pos_time_layernorm %s B=%d L=%d" % (_ln_add_id(case), B, L), "out", read(out, rows * H, "out").reshape(rows, H),
                sr.layernorm(v, gamma, beta, EPS, ot, sr.ln_depth(H)))


# ------------------------------------------------------------------------------------------------------------------ 13. LayerNorm, panels
PANEL4_H = (128, 256, 384, 512, 768)           # ln_panel4_kernel<4, 8, 12, 16, 24>
PANEL16_H = (64, 128, 256, 384, 512, 768)      # ln_panel_kernel<2, 4, 8, 12, 16, 24> (H = 64 always; the others with the 4-row form switched off)
PANEL_ROWS = (1, 17, 67)
PANEL_ADD_BL = ((1, 1), (17, 1), (23, 3))      # rows 1, 17, 69 (L = 3: a wave's rows span batch items)
# (H, form, add: 0 | "bf16" | "f32", emb_row given)
PANEL_CASES = ([(H, "panel4", add, H % 256 == 0) for H in PANEL4_H for add in (0, "bf16", "f32")] + [(64, "panel16", add, 1) for add in (0, "bf16", "f32")])
PANEL16_DBG_CASES = [(H, "panel16", add, H % 256 != 0) for H in PANEL16_H[1:] for add in (0, "bf16", "f32")]


def _panel_id(c):
    return "H%d-%s-add_%s-embrow%d" % (c[0], c[1], c[2], int(c[3]))


def panel_case_key(c):
    H, form, add, _ = c
    return sc.ln_key("%s<%d, ADD>" % ("ln_panel4_kernel" if form == "panel4" else "ln_panel_kernel", H // 32), "f32" if add == "f32" else "bf16", None,
                     int(bool(add)))


def _panel_case(c, L_):
    H, form, add, rows_given = c
    nkb = H // 32
    depth = sr.ln_depth(H, form)
    for B, L in (PANEL_ADD_BL if add else [(r, 1) for r in PANEL_ROWS]):
        rows = B * L
        ldx, ldo = rows + 3, rows + 5
        xt = F32 if add == "f32" else BF16
        x, gamma, beta, pos, emb_t, rows_of = ln_add_inputs(B, L, H, xt, rows_given, 0, H * 5 + rows)
        if add == "f32":
            ldf = H + 8
            xbuf = torch.full((rows * ldf + 8,), NAN, dtype=torch.float32, device=DEV)
            xbuf[:rows * ldf].view(rows, ldf)[:, :H] = dev(x)
            ldx = ldf
        else:
            xbuf = dev(sr.to_panel(x, ldx), BF16)                      # (rows behind the last hold NaN)
        out = nans(nkb * ldo * 32, BF16)
        keep = [dev(pos), dev(emb_t), ints(rows_of) if rows_given else None, dev(gamma), dev(beta)]
        pd, ed, rd, gd, bd = keep
        if add:
            call = lambda: run(L_.mh_add_pos_time_layernorm_panel, xbuf.data_ptr(), ldx, int(add == "f32"), pd.data_ptr(), ed.data_ptr(), _lib.ptr(rd),
                               gd.data_ptr(), bd.data_ptr(), out.data_ptr(), ldo, B, L, H, EPS)
            v = sr.add_pos_time(x, pos, emb_t, rows_of, L)
        else:
            call = lambda: run(L_.mh_layernorm_panel, xbuf.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), out.data_ptr(), ldo, rows, H, EPS)
            v = x
        keys = recorded(call)
        assert keys == [panel_case_key(c)], keys
        compare("layernorm_panel %s rows=%d" % (_panel_id(c), rows), "out", read_panel(out, nkb, rows, ldo, "out"),
                sr.layernorm(v, gamma, beta, EPS, BF16, depth))


@pytest.mark.parametrize("case", PANEL_CASES, ids=_panel_id)
def test_layernorm_panel(case):
    _panel_case(case, lib())


@pytest.mark.parametrize("case", PANEL16_DBG_CASES, ids=_panel_id)
def test_layernorm_panel_16_row_form(case, dbg_lib):
    """the 16-row kernel at H >= 128: the debug library's switch (mh_layernorm_set_rows4), restored afterwards"""
    dbg_lib.mh_layernorm_set_rows4(0)
    try:
        _panel_case(case, dbg_lib)
    finally:
        dbg_lib.mh_layernorm_set_rows4(1)


@pytest.mark.parametrize("H", [96, 1024, 32])
def test_layernorm_panel_unsupported_width_writes_nothing(H):
    rows = 5
    x, out = torch.zeros((H // 32) * rows * 32 + 64, dtype=torch.bfloat16, device=DEV), nans((H // 32) * rows * 32, BF16)
    g = dev(np.ones(H))
    rc = rejected(lib().mh_layernorm_panel, x.data_ptr(), rows, g.data_ptr(), g.data_ptr(), out.data_ptr(), rows, rows, H, EPS)
    assert rc == MH_ERR_UNSUPPORTED
    assert rejected(lib().mh_layernorm_panel, None, rows, g.data_ptr(), g.data_ptr(), out.data_ptr(), rows, rows, 128, EPS) == MH_ERR_INVALID
    untouched(out, "layernorm_panel")
    # ... and leaves no launch note behind for the next launch to pick up
    t, o = dev(np.ones((4, 8))), nans(4)
    recs = sc.record(lambda: (rejected(lib().mh_layernorm_panel, x.data_ptr(), rows, g.data_ptr(), g.data_ptr(), out.data_ptr(), rows, rows, H, EPS),
                              run(lib().mh_row_sqnorm, t.data_ptr(), o.data_ptr(), 4, 8)))
    assert [(k, note) for k, note, _ in recs] == [("row_sqnorm_kernel", "")], recs


# ------------------------------------------------------------------------------------------------------------------ 14. argbest
# (n_tokens, V, E): every value of n in {1, 63, 65, 700}, V in {1, 63, 65, 729}, E in {1, 16, 63, 65, 128, 500}
ARG_CASES = [(1, 1, 1), (63, 63, 1), (65, 65, 16), (700, 729, 128), (63, 729, 63), (65, 63, 65), (1, 729, 500), (700, 65, 16), (65, 729, 65),
             (63, 65, 500), (700, 63, 63), (1, 65, 128)]
MFMA_CASES = ARG_CASES + [(65, 729, 20), (63, 65, 20)]
SCORES_CASES = [(65, 65, 16), (700, 729, 128), (700, 65, 16), (1, 65, 128)]
NEAR_CAP = 0.01


def arg_inputs(n, V, E):
    x, table, bias, first_of, pairs = sr.argbest_inputs(n, V, E, n * 7 + V * 3 + E)
    tnorm = (table.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    return x, table, bias, tnorm, first_of


def _margin(name, scores, bound, got, first_of, n):
    near, bad = sr.argbest_check(scores, bound, got, first_of)
    print("STEP-MATRIX %s near-tie rows %d of %d" % (name, near, n))
    assert not bad, name + ": " + "; ".join(bad)
    assert near <= NEAR_CAP * n, "%s: %d of %d rows in the near-tie class" % (name, near, n)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,V,E", ARG_CASES)
def test_vocab_argmax(n, V, E, mode):
    x, table, bias, tnorm, first_of = arg_inputs(n, V, E)
    idx = minus(n)
    xd, td, ad = dev(x), dev(table), dev(tnorm if mode == 0 else bias)
    fn = lib().mh_round_to_embedding if mode == 0 else lib().mh_logits_argmax
    keys = recorded(lambda: run(fn, xd.data_ptr(), td.data_ptr(), ad.data_ptr(), idx.data_ptr(), n, E, V))
    assert keys == ["vocab_argmax_kernel<%d>" % mode]
    scores, bound = sr.round_scores(x, table, tnorm) if mode == 0 else sr.logit_scores(x, table, bias)
    _margin("vocab_argmax<%d> n=%d V=%d E=%d" % (mode, n, V, E), scores, bound, read(idx, n, "idx"), first_of, n)


def _ws_views(ws, n, E, V):
    """the workspace of mh_round_to_embedding_mfma: |x_n|^2 [n], then the partial scores and indices [n, slots], each 256-byte aligned"""
    ns = int(lib().mh_round_slots(V))
    al = lambda b: (b + 255) & ~255
    o1 = al(n * 4)
    o2 = o1 + al(n * ns * 4)
    raw = ws.cpu()
    rown = raw[:n * 4].view(torch.float32).numpy()
    pbest = raw[o1:o1 + n * ns * 4].view(torch.float32).numpy().reshape(n, ns)
    pidx = raw[o2:o2 + n * ns * 4].view(torch.int32).numpy().reshape(n, ns)
    return rown, pbest, pidx, ns


@pytest.mark.parametrize("n,V,E", MFMA_CASES)
def test_round_to_embedding_mfma(n, V, E):
    """a workspace of exactly mh_round_workspace_bytes followed by a guard; E % 16 != 0 goes through the padded copy; the row norms
    (row_sqnorm_f32_kernel) against float64; argbest_reduce_kernel against the numpy fold of the partials it read"""
    x, table, bias, tnorm, first_of = arg_inputs(n, V, E)
    Ep = (E + 15) // 16 * 16
    tpad = np.zeros((V, Ep), dtype=np.float32)
    tpad[:, :E] = table
    nbytes = int(lib().mh_round_workspace_bytes(n, E, V))
    ws = torch.full((nbytes + 1024,), 0xFF, dtype=torch.uint8, device=DEV)
    idx = minus(n)
    xd, td, nd = dev(x), dev(tpad), dev(tnorm)
    keys = recorded(lambda: run(lib().mh_round_to_embedding_mfma, xd.data_ptr(), td.data_ptr(), nd.data_ptr(), idx.data_ptr(), n, E, V, ws.data_ptr(), nbytes))
    assert [k for k in keys] == (["cast_pad_kernel<float>"] if Ep != E else []) + ["row_sqnorm_f32_kernel", "argbest_reduce_kernel"], keys
    assert bool((ws[nbytes:] == 0xFF).all()), "written behind the workspace"
    got = read(idx, n, "idx")
    rown, pbest, pidx, ns = _ws_views(ws, n, E, V)
    name = "round_to_embedding_mfma n=%d V=%d E=%d" % (n, V, E)
    compare(name, "row norms", rown, sr.row_sqnorm(x))
    exact(name, "argbest_reduce against the numpy fold", got, sr.fold_slots(pbest, pidx))
    scores, bound = sr.round_scores(x, table, tnorm, K=Ep)
    _margin(name, scores, bound, got, first_of, n)
    # the same partials through the update kernel's own fold
    B, L, E8 = 1, n, 8
    d = _epi_inputs(("p", "vec", "idx", 0, "none", 0, 0, 0, 0), B, L, E8, V)
    case = (0, ns, 1, "none", "none", 0, 0)
    _, res = _slots_call(case, B, L, E8, V, d, pbest, pidx, None, None)
    exact(name, "round_idx_out of mh_step_epilogue_slots on the same partials", res[3], got)


@pytest.mark.parametrize("n,V,E", SCORES_CASES)
def test_round_scores_then_numpy_fold(n, V, E):
    x, table, bias, tnorm, first_of = arg_inputs(n, V, E)
    ns = int(lib().mh_round_slots(V))
    xn = (x.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    pb, pi = nans(n * ns), minus(n * ns)
    xd, xnd, td, nd = dev(x), dev(xn), dev(table), dev(tnorm)
    run(lib().mh_round_scores, xd.data_ptr(), xnd.data_ptr(), td.data_ptr(), nd.data_ptr(), pb.data_ptr(), pi.data_ptr(), n, E, V)
    pbest, pidx = read(pb, n * ns, "pbest").reshape(n, ns), read(pi, n * ns, "pidx").reshape(n, ns)
    assert not np.isnan(pbest).any(), "every slot of every row is written"
    scores, bound = sr.round_scores(x, table, tnorm)
    _margin("round_scores n=%d V=%d E=%d" % (n, V, E), scores, bound, sr.fold_slots(pbest, pidx), first_of, n)


# ------------------------------------------------------------------------------------------------------------------ 15. head
HEAD_BL = ((1, 1), (3, 21), (5, 13), (8, 25))          # rows 1, 63, 65, 200; no L divides the 64 (32) rows of a block
HEAD_E = ((128, 128), (100, 128), (4, 32), (64, 64))
HEAD_CASES = [(H, E, Ep, (i + j) % 2) for i, H in enumerate((256, 512, 768)) for j, (E, Ep) in enumerate(HEAD_E)]
HEAD_KERNEL = {256: "head_fused_kernel<256>", 512: "head_fused_kernel<512>", 768: "head_fused_kernel<768, 32>"}


def head_inputs(H, E, Ep, B, L, rows_given):
    g = sr.rng(H + E + B * L)
    x = (0.5 * g.standard_normal((B * L, E))).astype(np.float32)
    w0, b0 = sr.dense_inputs(H, E, H + E, pad_to=Ep)
    w2, b2 = sr.dense_inputs(H, H, H + E + 1)
    pos, emb_t, rows_of = sr.pos_time_inputs(B, L, H, H + B, rows_given)
    gamma = (1.0 + 0.2 * g.standard_normal(H)).astype(np.float32)
    beta = (0.2 * g.standard_normal(H)).astype(np.float32)
    return x, w0, b0, w2, b2, pos, emb_t, rows_of, gamma, beta


def wpanel(w):
    """[rows, K] bf16 values -> device K32 panels [K / 32][rows][32]"""
    return dev(sr.to_panel(w, w.shape[0]), BF16)


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "H%d-E%d-Epad%d-embrow%d" % c)
def test_up_proj_ln_fused(case):
    H, E, Ep, rows_given = case
    assert lib().mh_up_proj_ln_fused_supported(E, Ep, H) == 1
    for B, L in HEAD_BL:
        rows = B * L
        ldo = rows + 3
        x, w0, b0, w2, b2, pos, emb_t, rows_of, gamma, beta = head_inputs(H, E, Ep, B, L, rows_given)
        keep = [dev(x), wpanel(w0), dev(b0), wpanel(w2), dev(b2), dev(pos), dev(emb_t), ints(rows_of) if rows_given else None, dev(gamma), dev(beta)]
        xd, w0d, b0d, w2d, b2d, pd, ed, rd, gd, bd = keep
        out = nans((H // 32) * ldo * 32, BF16)
        keys = recorded(lambda: run(lib().mh_up_proj_ln_fused, xd.data_ptr(), E, Ep, w0d.data_ptr(), b0d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), pd.data_ptr(),
                                    ed.data_ptr(), _lib.ptr(rd), gd.data_ptr(), bd.data_ptr(), EPS, out.data_ptr(), ldo, B, L, H))
        assert keys == [HEAD_KERNEL[H]], keys
        compare("up_proj_ln_fused H=%d E=%d rows=%d" % (H, E, rows), "out", read_panel(out, H // 32, rows, ldo, "out"),
                sr.head(x, Ep, w0, b0, w2, b2, pos, emb_t, rows_of, L, gamma, beta, EPS))


# ------------------------------------------------------------------------------------------------------------------ 16. tail
TAIL_ROWS = (1, 63, 65, 200, 1000)
TAIL_CASES = [(256, 64), (512, 128), (768, 128)]
TAIL_KERNEL = {256: "tail_fused_kernel<256>", 512: "tail_fused_kernel<512>", 768: "tail_fused_kernel<768, 0, 32>"}
ROUND_KERNEL = {512: "tail_fused_kernel<512, 6>", 768: "tail_fused_kernel<768, 4, 32>"}


def tail_inputs(H, E, rows):
    g = sr.rng(H * 3 + E + rows)
    X = sr.bf16_round(g.standard_normal((rows, H)).astype(np.float32))
    w0, b0 = sr.dense_inputs(H, H, H + 11)
    w2, b2 = sr.dense_inputs(E, H, H + 12)
    return X, w0, b0, w2, b2


@pytest.mark.parametrize("H,E", TAIL_CASES)
def test_down_proj_fused(H, E):
    assert lib().mh_down_proj_fused_supported(E, H) == 1
    for rows in TAIL_ROWS:
        for with_sq in ((1,) if rows != 65 else (0, 1)):
            ldx = rows + 3
            X, w0, b0, w2, b2 = tail_inputs(H, E, rows)
            keep = [dev(sr.to_panel(X, ldx), BF16), wpanel(w0), dev(b0), wpanel(w2), dev(b2)]
            Xd, w0d, b0d, w2d, b2d = keep
            out, sq = nans(rows * E), nans(rows)
            keys = recorded(lambda: run(lib().mh_down_proj_fused, Xd.data_ptr(), ldx, w0d.data_ptr(), b0d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), out.data_ptr(),
                                        sq.data_ptr() if with_sq else None, rows, E, H))
            assert keys == [TAIL_KERNEL[H]], keys
            got = read(out, rows * E, "out").reshape(rows, E)
            name = "down_proj_fused H=%d rows=%d" % (H, rows)
            compare(name, "out", got, sr.tail(X, w0, b0, w2, b2))
            compare(name, "sqnorm of the rows written", read(sq, rows if with_sq else 0, "sqnorm"), sr.row_sqnorm(got) if with_sq else (np.zeros(0), np.zeros(0)))


# (H, ddim, noise, mask, pred, mean, clip)
UPD_CASES = [(512, 0, "rng", "row", 1, 1, 1), (512, 1, "given", "elem", 1, 0, 1), (512, 0, "none", "none", 0, 0, 0), (768, 1, "rng", "elem", 0, 0, 1),
             (768, 0, "given", "row", 1, 1, 0), (768, 1, "none", "none", 1, 0, 1), (512, 0, "given", "elem", 0, 1, 1), (512, 1, "rng", "row", 1, 0, 0)]
ROUND_ONLY_CASES = [(512, 729), (768, 729), (512, 641), (768, 768)]


def _upd_id(c):
    return "H%d-%s-noise_%s-mask%s-pred%d-mean%d-clip%d" % (c[0], "ddim" if c[1] else "p", c[2], c[3], c[4], c[5], c[6])


def upd_case_key(c):
    return sc.tail_key(ROUND_KERNEL[c[0]], 1, c[1], c[2], c[3])


@functools.lru_cache(maxsize=None)
def round_table(H, V, rows):
    """the embedding table of a rounding case: N(0, 0.6^2) rows, and - as in the argbest cases, where x is a table row plus noise - up to 600
    of them replaced by a row of the float32 restatement of this very down-projection plus 0.05-scaled noise, at scattered indices: those
    token rows have one clear nearest table row whatever the last bits of the kernel's rows are; the others (rows > 600) meet the table
    as random points do, within the 1 % cap (tests/test_step_bound_cpu.py checks the share per case).  A tenth of the entries lie
    outside [-1, 1], for the clip."""
    g = sr.rng(V + rows + H)
    table = (0.6 * g.standard_normal((V, 128))).astype(np.float32)
    y = sr.dense_emulate(*tail_inputs(H, 128, rows))
    m = min(rows, 600)
    at = g.permutation(V)[:m]
    table[at] = y[:m] + (0.05 * g.standard_normal((m, 128))).astype(np.float32)
    return table


def _tail_round(H, V, rows, upd_case, with_sq=True):
    """mh_down_proj_round_fused on `rows` rows (pitch rows + 3): rows, their norms, their nearest table rows; with `upd_case` the update"""
    E = 128
    ldx = rows + 3
    X, w0, b0, w2, b2 = tail_inputs(H, E, rows)
    table = round_table(H, V, rows)
    keep = [dev(sr.to_panel(X, ldx), BF16), wpanel(w0), dev(b0), wpanel(w2), dev(b2), dev(table)]
    Xd, w0d, b0d, w2d, b2d, td = keep
    buf = torch.empty(int(lib().mh_round_split_bytes(E, V)), dtype=torch.uint8, device=DEV)
    run(lib().mh_round_split_table, td.data_ptr(), None, V, E, buf.data_ptr())
    out, sq, idx = nans(rows * E), nans(rows), minus(rows)
    res = dict(table=table)
    u = None
    if upd_case is not None:
        _, ddim, noise, form_m, pred, mean, clip = upd_case
        B, L = 1, rows
        d = _epi_inputs(("ddim" if ddim else "p", "vec", "idx", clip, form_m, 0, 1, 1, 1), B, L, E, V)
        d["table"] = table
        guard = 5
        xbuf = nans((rows + guard) * E)
        xbuf[:rows * E] = dev(d["xt"]).view(-1)
        predb, meanb = nans(rows * E), nans(rows * E)
        counter = torch.tensor([RNG_STEP], dtype=torch.int32, device=DEV)
        r = _lib.StepRng()
        r.seed, r.stream_id, r.bound, r.step_counter, r.first_elem = RNG_DESC["seed"], RNG_DESC["stream"], RNG_DESC["bound"], counter.data_ptr(), RNG_DESC["first"]
        if noise == "rng":
            nzb = nans(rows * E + 4)
            run(lib().mh_trunc_normal_at, nzb.data_ptr(), rows * E, RNG_DESC["first"], RNG_DESC["bound"], RNG_DESC["seed"], RNG_DESC["stream"], counter.data_ptr())
            d["nz"] = host(nzb[:rows * E]).reshape(B, L, E)
        keep += [dev(d["nz"]), dev(d["coef"]), ints(d["mask"]) if d["mask"] is not None else None, dev(d["xs"])]
        nz_d, coef_d, mask_d, xs_d = keep[-4:]
        u = _lib.StepUpdate()
        u.x, u.x_start, u.mask, u.mask_per_elem = xbuf.data_ptr(), _lib.ptr(xs_d) if mask_d is not None else None, _lib.ptr(mask_d), int(form_m == "elem")
        u.table, u.coef, u.clip, u.ddim = td.data_ptr(), coef_d.data_ptr(), clip, ddim
        u.pred_xstart, u.mean_out = predb.data_ptr() if pred else None, meanb.data_ptr() if mean else None
        u.noise = nz_d.data_ptr() if noise == "given" else None
        u.rng = C.pointer(r) if noise == "rng" else None
        res.update(d=d, xbuf=xbuf, predb=predb, meanb=meanb, guard=guard)
    keys = recorded(lambda: run(lib().mh_down_proj_round_fused, Xd.data_ptr(), ldx, w0d.data_ptr(), b0d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), out.data_ptr(),
                                sq.data_ptr() if with_sq else None, buf.data_ptr(), V, idx.data_ptr(), C.byref(u) if u is not None else None, rows, E, H))
    res.update(keys=keys, out=read(out, rows * E, "out").reshape(rows, E), sq=read(sq, rows if with_sq else 0, "sqnorm"), idx=read(idx, rows, "idx"),
               ref=sr.tail(X, w0, b0, w2, b2))
    return res


def _check_round(name, res, V, rows):
    compare(name, "out", res["out"], res["ref"])
    if res["sq"].size:
        compare(name, "sqnorm of the rows written", res["sq"], sr.row_sqnorm(res["out"]))
    scores, bound = sr.round_scores(res["out"], res["table"], None, split=True)
    _margin(name, scores, bound, res["idx"], None, rows)


@pytest.mark.parametrize("H,V", ROUND_ONLY_CASES)
def test_down_proj_round_fused(H, V):
    assert lib().mh_down_proj_round_supported(128, H, V) == 1
    for rows in TAIL_ROWS:
        res = _tail_round(H, V, rows, None, with_sq=rows != 63)
        assert res["keys"] == [sc.tail_key(ROUND_KERNEL[H], 0)], res["keys"]
        _check_round("down_proj_round_fused H=%d V=%d rows=%d" % (H, V, rows), res, V, rows)


@pytest.mark.parametrize("case", UPD_CASES, ids=_upd_id)
def test_down_proj_round_fused_with_update(case):
    """the update inside the tail: given the idx_out the kernel wrote, x, pred and mean equal the numpy float32 reference of the update
    kernels bit for bit, and mh_step_epilogue_slots(nslots = 0, pidx = idx_out) on the same operands; the rows behind `rows` of x are
    untouched"""
    H, ddim, noise, form_m, pred, mean, clip = case
    V, E = 729, 128
    for rows in (65, 200) if H == 512 else (63, 200):
        res = _tail_round(H, V, rows, case)
        name = "down_proj_round_fused+update %s rows=%d" % (_upd_id(case), rows)
        assert res["keys"] == [upd_case_key(case)], res["keys"]
        _check_round(name, res, V, rows)
        d, idx = res["d"], res["idx"]
        ref = sr.step_update(res["table"][idx.reshape(1, rows)], d["xt"], d["nz"] if noise != "none" else None, d["coef"], clip, bool(ddim), d["mask"], d["xs"])
        exact(name, "x", read(res["xbuf"], rows * E, "x (guard rows)").reshape(1, rows, E), ref[0])
        exact(name, "pred_xstart", read(res["predb"], rows * E if pred else 0, "pred").reshape(-1), ref[1].reshape(-1) if pred else np.zeros(0, np.float32))
        exact(name, "mean", read(res["meanb"], rows * E if (mean and not ddim) else 0, "mean").reshape(-1),
              ref[2].reshape(-1) if (mean and not ddim) else np.zeros(0, np.float32))
        slot_case = (ddim, 0, 0, "given" if noise != "none" else "none", form_m, 0, clip)
        _, got = _slots_call(slot_case, 1, rows, E, V, d, None, idx.reshape(rows, 1), None, None)
        exact(name, "x against mh_step_epilogue_slots(nslots = 0)", got[0], ref[0])


def test_tail_update_error_paths_write_nothing():
    H, E, V, rows = 512, 128, 729, 8
    X, w0, b0, w2, b2 = tail_inputs(H, E, rows)
    keep = [dev(sr.to_panel(X, rows), BF16), wpanel(w0), dev(b0), wpanel(w2), dev(b2), dev(np.zeros((V, E))), dev(sr.coef_table("p")[[3]])]
    Xd, w0d, b0d, w2d, b2d, td, cd = keep
    buf = torch.zeros(int(lib().mh_round_split_bytes(E, V)), dtype=torch.uint8, device=DEV)
    out, idx, x = nans(rows * E), minus(rows), nans(rows * E + 4)
    u = _lib.StepUpdate()
    u.x, u.table, u.coef = x.data_ptr() + 4, td.data_ptr(), cd.data_ptr()          # x off its 16-byte boundary
    rejected(lib().mh_down_proj_round_fused, Xd.data_ptr(), rows, w0d.data_ptr(), b0d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), out.data_ptr(), None, buf.data_ptr(),
             V, idx.data_ptr(), C.byref(u), rows, E, H)
    r = _lib.StepRng()
    r.seed, r.bound, r.first_elem = 1, 1.0, 2
    u.x, u.rng = x.data_ptr(), C.pointer(r)                                         # first_elem % 4 != 0
    rejected(lib().mh_down_proj_round_fused, Xd.data_ptr(), rows, w0d.data_ptr(), b0d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), out.data_ptr(), None, buf.data_ptr(),
             V, idx.data_ptr(), C.byref(u), rows, E, H)
    for t, what in ((out, "out"), (idx, "idx"), (x, "x")):
        untouched(t, what)
