"""GPU: mhv_dpmpp_epilogue (csrc/solver.hip) through the C ABI (include/musehip_solver.h).  Every output starts NaN-filled between guard
bands and every element is judged bit for bit against the fp32 restatement tests/solver_ref.py; a second check holds it to the float64
value of the rule on the fp32 coefficients within 4 * 2^-24 * (|a x_t| + |b v| + |c p|): three product roundings plus two sums."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import solver_ref as sr  # noqa: E402
from musediffusion_amd import _lib, ops  # noqa: E402
from musediffusion_amd.models.diffusion import get_named_beta_schedule, GaussianDiffusion  # noqa: E402
from test_solver_cpu import c_abi_refusals, call_with  # noqa: E402

DEV = "cuda"
GUARD = 64                      # floats: a multiple of 4, so the guarded region keeps the allocation's 16-byte alignment
V = 729
ACP = GaussianDiffusion(betas=get_named_beta_schedule("sqrt", 50), predict_xstart=True).alphas_cumprod
TABLE = sr.table_f32(ACP, 5, 2)                 # T = 50, gap 5: row 49 is the first step (c == 0), row 4 the clean target
ROW_HIST, ROW_FIRST, ROW_CLEAN = 29, 49, 4
assert TABLE[ROW_HIST, 2] != 0 and TABLE[ROW_FIRST, 2] == 0 and tuple(TABLE[ROW_CLEAN, :3]) == (0.0, 1.0, 0.0)


class Buf:
    """`n` floats between two NaN guard bands, NaN-filled or holding `init`; shift: floats by which the region is moved off 16 bytes"""

    def __init__(self, n, init=None, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((n + 2 * GUARD + 4,), float("nan"), device=DEV)
        if init is not None:
            self.buf[self.lo:self.lo + n] = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)).to(DEV)
        self.ptr = self.buf.data_ptr() + 4 * self.lo

    def get(self, shape):
        host = self.buf.cpu().numpy()
        assert np.isnan(host[:self.lo]).all() and np.isnan(host[self.lo + self.n:]).all(), "guard band written"
        return host[self.lo:self.lo + self.n].reshape(shape)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def make_inputs(g, B, L, E, source, mask_form, cpb, nslots):
    n = B * L
    d = dict(B=B, L=L, E=E, source=source, mask_form=mask_form, cpb=cpb)
    d["x_t"] = g.standard_normal((B, L, E)).astype(np.float32)
    d["prev"] = g.standard_normal((B, L, E)).astype(np.float32)
    d["x_start"] = g.standard_normal((B, L, E)).astype(np.float32)
    table = (1.2 * g.standard_normal((V, E))).astype(np.float32)
    table[::7, 0], table[3::7, -1], table[5::11, E // 2] = 1.0, -1.0, 1.0 + 2.0 ** -23        # exactly +-1 and one ulp beyond
    d["table"] = table
    if source == "model":
        mo = (1.5 * g.standard_normal((B, L, E))).astype(np.float32)
        flat = mo.reshape(-1)
        flat[::5], flat[2::9], flat[4::13] = 1.0, -1.0, -1.0 - 2.0 ** -23
        d["model_out"], d["v"] = mo, mo
    elif source == "idx":
        d["round_idx"] = g.integers(0, V, n).astype(np.int32)
        d["v"] = table[d["round_idx"]].reshape(B, L, E)
    else:
        ns = nslots if source == "slots" else 0
        d["nslots"] = ns
        if ns:
            pb = g.integers(-3, 4, (n, ns)).astype(np.float32)              # few values: ties in every row
            pi = g.integers(0, V, (n, ns)).astype(np.int32)
            pb[0] = -np.inf                                                  # a row of -inf scores: all tie, the smallest index wins
            if n > 1:
                pb[1], pi[1, 0], pi[1, -1] = 2.0, 700, 11                    # all equal: the smallest index wins, wherever it sits
            if n > 2:
                pb[2, 0], pb[2, 1:] = np.nan, -np.inf                        # NaN never wins
            if n > 3:
                pb[3] = np.nan                                               # ... and a row of nothing else takes index 0
            d["pbest"], d["pidx"] = pb, pi
        else:
            d["pidx"] = g.integers(0, V, n).astype(np.int32)
        d["v"] = table[sr.fold_slots(d.get("pbest"), d["pidx"], ns)].reshape(B, L, E)
    if cpb:
        rows = [ROW_HIST, ROW_FIRST, ROW_CLEAN, 14][:B]
        d["coef"] = TABLE[rows]
    else:
        d["coef"] = TABLE[ROW_HIST]
    if mask_form == "row":
        m = g.integers(0, 2, (B, L)).astype(np.int32)
        m[0], m[-1, :] = 0, (1 if B > 1 else m[-1, :])                       # an all-anchored batch row and (B > 1) a none-anchored one
        m[B // 2, L // 2] = 2                                                # only 0 anchors
        d["mask"], d["anchored"] = m, np.broadcast_to((m == 0)[:, :, None], (B, L, E))
    elif mask_form == "elem":
        m = g.integers(0, 2, (B, L, E)).astype(np.int32)
        m[0, 0], m[-1, -1] = 0, 1
        d["mask"], d["anchored"] = m, m == 0
    return d


def launch(d, clip=1, hist="sep", alias_out=False, shift=0, prev=None, twice=False):
    """-> (out, pred) as numpy; hist: none | sep | alias (the history IS pred_xstart); shift: every float tensor moved off 16 bytes"""
    B, L, E = d["B"], d["L"], d["E"]
    n = B * L * E
    keep, ints = [], []

    def inp(a):
        b = Buf(np.asarray(a).size, a, shift)
        keep.append(b)
        return b.ptr

    prev = d["prev"] if prev is None else prev
    x_t = Buf(n, d["x_t"], shift)
    out = x_t if alias_out else Buf(n, None, shift)
    pred = Buf(n, prev if hist == "alias" else None, shift)
    prev_p = None if hist == "none" else (pred.ptr if hist == "alias" else inp(prev))
    P = lambda name, dt: (ints.append(dev(d[name], dt)) or ints[-1].data_ptr()) if name in d else None  # noqa: E731
    mo_p = inp(d["model_out"]) if "model_out" in d else None
    tab_p = inp(d["table"]) if d["source"] != "model" else None
    xs_p = inp(d["x_start"]) if "mask" in d else None
    pb_p = inp(d["pbest"]) if "pbest" in d else None
    coef = dev(d["coef"], np.float32)
    args = (mo_p, x_t.ptr, prev_p, P("round_idx", np.int32), pb_p, P("pidx", np.int32), d.get("nslots", 0), tab_p, coef.data_ptr(), int(d["cpb"]),
            int(clip), P("mask", np.int32), int(d["mask_form"] == "elem"), xs_p, out.ptr, pred.ptr, B, L * E, E, _lib.current_stream())
    for _ in range(2 if twice else 1):
        _lib.check(_lib.lib().mhv_dpmpp_epilogue(*args), "mhv_dpmpp_epilogue")
    torch.cuda.synchronize()
    for b in keep:
        b.get((-1,))                                                         # no input's guard band was written either
    return out.get((B, L, E)), pred.get((B, L, E))


def reference(d, clip, hist, prev=None):
    prev = None if hist == "none" else (d["prev"] if prev is None else prev)
    return sr.update_f32(d["x_t"], d["v"], prev, d["coef"], clip, d.get("anchored"), d["x_start"]), prev


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check(d, clip=1, hist="sep", alias_out=False, shift=0, prev=None, what=""):
    got_out, got_pred = launch(d, clip, hist, alias_out, shift, prev)
    (want_out, want_pred), p = reference(d, clip, hist, prev)
    tag = (what, d["B"], d["L"], d["E"], d["source"], d["mask_form"], d["cpb"], clip, hist, alias_out, shift)
    assert np.array_equal(bits(got_pred), bits(want_pred)), (tag, "pred_xstart", np.argwhere(bits(got_pred) != bits(want_pred))[:4].tolist())
    assert np.array_equal(bits(got_out), bits(want_out)), (tag, "out", np.argwhere(bits(got_out) != bits(want_out))[:4].tolist())
    # against float64: wherever the update ran (not anchored) and everything is finite
    val, bound = sr.update_f64(d["x_t"], d["v"], p, d["coef"], clip)
    free = np.isfinite(val) & (~d["anchored"] if "anchored" in d else True)
    assert (np.abs(got_out.astype(np.float64) - val)[free] <= bound[free]).all(), (tag, "float64 bound")
    if "anchored" in d:
        assert np.array_equal(bits(got_out[d["anchored"]]), bits(d["x_start"][d["anchored"]]))
    return got_out, got_pred


SHAPES = list(itertools.product((1, 2, 3), (1, 5, 64)))
VARIANTS = list(itertools.product(("none", "row", "elem"), (0, 1), ("none", "sep", "alias"), (0, 1)))      # mask, cpb, hist, clip


@pytest.mark.parametrize("E", [4, 16, 100, 5, 6])
def test_every_path_bit_for_bit(E):
    """E % 4 == 0: the 4-wide kernel with all four x0 sources; E = 5, 6: the scalar kernel (model and index sources).  The full product
    of mask form x coefficient rows x history x clip on one shape, a rotation of it over the others."""
    g = np.random.default_rng(100 + E)
    nslots = int(_lib.lib().mh_round_slots(V))
    assert nslots > 1
    sources = ("model", "idx", "slots", "slots0") if E % 4 == 0 else ("model", "idx")
    n = 0
    for (B, L), source in itertools.product(SHAPES, sources):
        full = (B, L) == (3, 5)
        picks = VARIANTS if full else [VARIANTS[(7 * n + k * 5) % len(VARIANTS)] for k in range(4)]
        for mask_form, cpb, hist, clip in picks:
            d = make_inputs(g, B, L, E, source, mask_form, cpb, nslots)
            check(d, clip, hist, alias_out=bool((n + clip) % 2))
            n += 1


@pytest.mark.parametrize("source", ["model", "idx"])
def test_four_wide_and_scalar_paths_give_the_same_bits(source):
    """the same data through both kernels: moving every float tensor 4 bytes off a 16-byte boundary sends the launch to the scalar kernel"""
    g = np.random.default_rng(7)
    for mask_form, cpb in (("none", 0), ("row", 1), ("elem", 0)):
        d = make_inputs(g, 3, 5, 16, source, mask_form, cpb, 0)
        a = check(d, 1, "sep", shift=0, what="aligned")
        b = check(d, 1, "sep", shift=1, what="misaligned")
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
        seen = launches_of(lambda: (launch(d, shift=0), launch(d, shift=1)))
        assert [k.split("<")[0] for k, _ in seen] == ["dpmpp_epilogue4_kernel", "dpmpp_epilogue_kernel"], seen


def launches_of(fn):
    import gemm_census as gc
    return [(k, note) for k, note, _ in gc.record_family(fn, lambda kernel, note: " ".join(kernel.strip().strip("()").split()))
            if k.startswith("dpmpp_")]


def test_launch_notes_name_the_runtime_path():
    g = np.random.default_rng(3)
    nslots = int(_lib.lib().mh_round_slots(V))
    want = []
    def go():
        for source, mask_form, cpb, hist in (("model", "none", 0, "none"), ("idx", "row", 1, "sep"), ("slots", "elem", 0, "alias"),
                                             ("slots0", "none", 0, "alias")):
            launch(make_inputs(g, 2, 5, 8, source, mask_form, cpb, nslots), hist=hist)
            x0 = "slots" if source.startswith("slots") else source
            want.append(("dpmpp_epilogue4_kernel<X0_%s>" % x0.upper(),                   # (the recorder keeps the launch's own text)
                         "x0=%s mask=%s cpb=%d hist=%s fold=%d" % (x0, mask_form, cpb, hist, source == "slots")))
    seen = launches_of(go)
    assert seen == want, (seen, want)


def test_history_is_not_read_where_c_is_zero_and_propagates_where_it_is_not():
    g = np.random.default_rng(11)
    for E, source in ((16, "slots"), (16, "model"), (5, "idx")):
        nslots = int(_lib.lib().mh_round_slots(V)) if source == "slots" else 0
        # c == 0 (the first step's row, shared; and a per-batch mix): a NaN-filled history, separate or in place, and no NaN comes out
        d = make_inputs(g, 3, 5, E, source, "none", 0, nslots)
        d["coef"] = TABLE[ROW_FIRST]
        nan = np.full_like(d["prev"], np.nan)
        for hist in ("sep", "alias"):
            out, pred = check(d, 1, hist, prev=nan, what="NaN history")
            assert np.isfinite(out).all() and np.isfinite(pred).all()
        d = make_inputs(g, 3, 5, E, source, "none", 1, nslots)                # rows HIST, FIRST, CLEAN: NaN only under the c == 0 rows
        mixed = d["prev"].copy()
        mixed[1:] = np.nan
        out, _ = check(d, 1, "sep", prev=mixed, what="mixed history")
        assert np.isfinite(out).all()
        # c != 0: an inf in the history reaches exactly its own element
        d = make_inputs(g, 3, 5, E, source, "none", 0, nslots)
        p = d["prev"].copy()
        p[1, 2, E - 1], p[2, 4, 0] = np.inf, -np.inf
        for hist in ("sep", "alias"):
            out, pred = check(d, 1, hist, prev=p, what="inf history")
            bad = ~np.isfinite(out)
            assert bad.sum() == 2 and bad[1, 2, E - 1] and bad[2, 4, 0] and np.isfinite(pred).all()
            assert out[1, 2, E - 1] == -np.inf and out[2, 4, 0] == np.inf     # (c < 0)


def test_repeated_call_gives_the_same_bits():
    g = np.random.default_rng(5)
    nslots = int(_lib.lib().mh_round_slots(V))
    for source, E in (("slots", 16), ("model", 6)):
        d = make_inputs(g, 2, 64, E, source, "row", 1, nslots)
        a, b = launch(d, hist="sep"), launch(d, hist="sep", twice=True)       # (separate outputs: the second call sees the same inputs)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("E,L", [(512, 5500), (5, 420000)])
def test_more_than_one_sweep_of_the_capped_grid(E, L):
    """8192 blocks of 256 threads: 2 097 152 groups of 4 (E = 512) or elements (E = 5) per sweep; the shapes are just past one sweep"""
    B = 3 if E == 512 else 1
    assert B * L * E // (4 if E % 4 == 0 else 1) > 8192 * 256
    g = np.random.default_rng(E)
    d = make_inputs(g, B, L, E, "idx", "row", int(B > 1), 0)
    check(d, 1, "alias", alias_out=True, what="grid-stride")


def test_ops_front_and_refusals_with_device_pointers():
    g = np.random.default_rng(2)
    d = make_inputs(g, 2, 5, 8, "idx", "row", 1, 0)
    t = lambda k, dt=np.float32: dev(d[k], dt)  # noqa: E731
    out, pred = ops.dpmpp_epilogue(None, t("x_t"), t("coef"), True, True, t("prev"), t("round_idx", np.int32), t("table"), None,
                                   t("mask", np.int32), t("x_start"))
    (want_out, want_pred), _ = reference(d, 1, "sep")
    assert np.array_equal(bits(out.cpu().numpy()), bits(want_out)) and np.array_equal(bits(pred.cpu().numpy()), bits(want_pred))
    buf = torch.zeros(256, device=DEV)
    lib = _lib.lib()
    for change, what in c_abi_refusals():
        assert call_with(lib, buf.data_ptr(), change, _lib.current_stream()) == _lib.MH_ERR_INVALID, what
        assert b"dpmpp_epilogue" in lib.mh_last_error(), what
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                     # nothing was launched
