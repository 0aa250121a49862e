"""Parity matrix of the optimizer kernels of csrc/train.hip: mh_adamw_ema_step, mh_grad_norm and mh_clip_grads called through the C ABI with
hand-built device tables (mh_opt_tensor and mh_opt_chunk rows as this module writes them, not FusedAdamWEMA's), against the float64
references, bounds and float32 restatements of tests/optim_ref.py.  Together with tests/test_train_matrix_gpu.py this covers every C entry
point of the file.

Rules of every case: every tensor's parameter, gradient, moments and EMA copies lie inside one larger allocation per kind (an "arena") with
NaN guard bands in front of and behind every tensor; `partial` and `out` are NaN-filled with slack; the EMA slots beyond n_ema point at
NaN-filled buffers; every arena is read back WHOLE and compared bit for bit with its expected image, so whatever lies outside the documented
output - guard bands, gradients, the parameter and moments of a NULL-gradient tensor, unused EMA slots - must be unchanged.  All base
pointers are 16-byte aligned and all chunk offsets multiples of 4 elements, as include/musehip.h requires.

What is asserted: m and v bit-equal to the float32 restatement and inside their float64 bounds; p inside dp, every element; every EMA copy
bit-equal to fl(fl(e r) + fl(p' (1 - r))) of the kernel's own p' and inside its float64 bound; every element of `partial` inside the
sum-of-squares bound of its chunk (exactly 0.0f for a NULL-gradient chunk) and out[0] inside the norm's; every gradient after the clip
bit-equal to fl(g coef) with coef formed in float32 from the norm the kernel wrote (the original bits when coef >= 1); a repeated call from
the same state gives the same bits.  A NaN gradient element stays in its own element's outputs.

Recorded, not asserted: the share of p elements that are bit-equal to the restatement (every case prints it in its OPTIM-MATRIX line).  p is
the one output that passes through a divide and a square root; HIP's are correctly rounded by default, so the share is expected to be 1 and
any other figure is a finding to look into at the divide or the square root.  Measured on an MI355X: 1.000000 in every case - p is
bit-equal to the restatement everywhere, and so are the chunk partials and the norm (the restatement sums in the kernels' order), so the
worst err / bound are the restatement's own: p 0.79, m 0.77, v 0.79, EMA copies 0.55 to 0.79, partials 0.24, norm 0.09.  Per case, and on
the parent commit's kernels as well (which fail the three NaN-norm clip cases and nothing else): profiles/optim_matrix.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as orf
import train_census as tc

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import check, current_stream, lib  # noqa: E402

DEV = "cuda"
F = np.float32
SLACK = 256
CHUNK_DTYPE = np.dtype([("tensor", "<i4"), ("count", "<i4"), ("offset", "<i8")])

# (table, NULL-gradient pattern, n_ema, step, weight decay, gradient kind)
ADAM_CASES = [
    ("host", "none", 3, 1, 0.01, "s1"),
    ("host", "first", 1, 2, 0.0, "s1e-4"),
    ("one", "last", 0, 1000, 0.1, "s1e-8"),
    ("one", "between", 4, 100000, 0.01, "s1e-12"),
    ("one", "none", 2, 1, 0.1, "s1e-12"),
    ("c8", "none", 2, 2, 0.01, "s1e6"),
    ("c8", "between", 1, 100000, 0.0, "s1e-4"),
    ("c1028", "allbut", 4, 1, 0.1, "s1"),
    ("c1028", "first", 0, 2, 0.1, "s1e-12"),
    ("shuffled", "span", 3, 1000, 0.01, "s1"),
    ("shuffled", "none", 4, 1, 0.0, "s1e-8"),
    ("host", "allbut", 2, 1000, 0.0, "s1e6"),
    ("host", "last", 4, 2, 0.01, "s1e-8"),
    ("host", "none", 4, 2, 0.01, "nonfinite"),
    ("c1028", "last", 3, 1, 0.01, "nonfinite"),
    ("shuffled", "between", 0, 100000, 0.1, "nonfinite"),
    ("n1", "none", 0, 1, 0.01, "s1"),
    ("n63", "first", 1, 2, 0.1, "s1e-4"),
    ("n64", "none", 2, 1000, 0.0, "s1"),
    ("n65", "last", 3, 100000, 0.01, "s1e-8"),
    ("n255", "none", 4, 1, 0.1, "s1e6"),
    ("n256", "first", 4, 2, 0.0, "s1"),
    ("n257", "none", 1, 1000, 0.01, "s1e-12"),
    ("n1000", "last", 2, 1, 0.01, "s1"),
]
# (table, NULL-gradient pattern, gradient kind)
NORM_CASES = [
    ("one", "none", "s1"), ("one", "first", "tail"), ("host", "none", "s1"), ("host", "between", "tail"), ("host", "last", "s1"),
    ("host", "none", "inf"), ("c8", "none", "chunk"), ("c8", "span", "s1"), ("c1028", "none", "tail"), ("c1028", "allbut", "s1"),
    ("c1028", "none", "small"), ("shuffled", "none", "s1"), ("shuffled", "first", "nan"), ("shuffled", "span", "chunk"),
    ("n1", "none", "s1"), ("n63", "none", "tail"), ("n64", "first", "s1"), ("n65", "none", "chunk"), ("n255", "last", "s1"),
    ("n256", "none", "s1"), ("n257", "none", "tail"), ("n1000", "none", "s1"), ("n1000", "first", "chunk"),
]
# (table, NULL-gradient pattern, gradient kind, mode): max_norm = half the norm ("above"), twice ("below"), the kernel's own norm + 1e-6f
# ("equal": coef is exactly 1), the float below that ("just_below": coef = 1 - 2^-24 or so); "inf" / "nan": such a gradient element
CLIP_CASES = [
    ("host", "none", "s1", "above"), ("host", "between", "s1", "below"), ("host", "none", "s1", "equal"), ("host", "none", "s1", "just_below"),
    ("one", "first", "tail", "above"), ("c8", "span", "s1", "above"), ("c1028", "allbut", "s1", "just_below"), ("c1028", "none", "small", "above"),
    ("c1028", "last", "small", "just_below"), ("c1028", "none", "small", "equal"), ("shuffled", "span", "chunk", "above"),
    ("shuffled", "none", "small", "below"), ("n257", "first", "tail", "above"), ("n1000", "none", "s1", "just_below"), ("n1", "none", "s1", "above"),
    ("host", "between", "inf", "above"), ("shuffled", "first", "inf", "above"),
    ("host", "between", "nan", "above"), ("shuffled", "first", "nan", "above"), ("n65", "none", "nan", "above"),
]


def _id(c):
    return "-".join(str(x) for x in c)


# ------------------------------------------------------------------------------------------------------------------ buffers
class Arena:
    """one allocation holding every tensor of a Layout at its 16-byte aligned offset, NaN everywhere else.  `flat` = the values in flat
    coordinates (None: the tensors are NaN too)"""

    def __init__(self, lay, flat=None):
        self.lay = lay
        self.image = np.full(lay.arena, np.nan, dtype=F)
        if flat is not None:
            self.image[lay.aidx] = flat
        self.t = torch.from_numpy(self.image.copy()).to(DEV)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, i):
        return self.t.data_ptr() + 4 * int(self.lay.offs[i])

    def reset(self):
        self.t.copy_(torch.from_numpy(self.image))

    def read(self, what, expect_flat=None):
        """the tensors' values in flat coordinates; everything around them must hold its initial bits (expect_flat: so must the tensors)"""
        a = self.t.cpu().numpy()
        want = self.image.copy()
        if expect_flat is None:
            want[self.lay.aidx] = a[self.lay.aidx]
        else:
            want[self.lay.aidx] = expect_flat
        bad = ~orf.same_bits(a, want)
        assert not bad.any(), "%s: %d elements differ from what they must hold, first at arena index %d (tensors start at %s)" % (
            what, int(bad.sum()), int(np.argmax(bad)), self.lay.offs.tolist()[:8])
        return a[self.lay.aidx]


class Tables:
    """device images of the mh_opt_tensor and mh_opt_chunk tables of a Layout over arenas p, g, m, v, e[0..3]"""

    def __init__(self, lay, p, g, m, v, e):
        rows = np.zeros((len(lay.sizes), 8), dtype=np.int64)
        for i in range(len(lay.sizes)):
            rows[i, :4] = p.ptr(i), (0 if i in lay.nulls else g.ptr(i)), m.ptr(i), v.ptr(i)
            rows[i, 4:] = [a.ptr(i) for a in e]
        assert not (rows & 15).any()
        ch = np.zeros(len(lay.chunks), dtype=CHUNK_DTYPE)
        ch["tensor"], ch["count"], ch["offset"] = lay.chunks.T
        self.tensors = torch.from_numpy(rows).to(DEV)
        self.chunks = torch.from_numpy(ch.view(np.uint8).copy()).to(DEV)
        self.n = len(lay.chunks)


def nans(n):
    return torch.full((int(n) + SLACK,), float("nan"), dtype=torch.float32, device=DEV)


def read(t, n, what):
    a = t.cpu().numpy()
    assert np.isnan(a[n:]).all(), "%s: written behind its %d elements" % (what, n)
    return a[:n]


def c_hparams(hp):
    s = _lib.OptHParams()
    for k in ("beta1", "beta2", "eps", "one_minus_beta1", "one_minus_beta2", "decay_mul", "step_size", "bias2_sqrt"):
        setattr(s, k, float(hp[k]))
        assert F(getattr(s, k)) == hp[k]
    s.n_ema = hp["n_ema"]
    for k in range(4):       # (slots beyond n_ema: a value that would show if a kernel used it)
        s.ema_rate[k] = float(hp["ema_rate"][k]) if k < hp["n_ema"] else 7.0
        s.ema_one_minus[k] = float(hp["ema_one_minus"][k]) if k < hp["n_ema"] else -3.0
    return s


def exact(case, name, got, want, mask=None):
    bad = ~orf.same_bits(got, want)
    if mask is not None:
        bad &= mask
    assert not bad.any(), "%s %s: %d of %d elements differ in bits, first at flat index %d: got %r want %r" % (
        case, name, int(bad.sum()), bad.size, int(np.argmax(bad)), got[int(np.argmax(bad))], want[int(np.argmax(bad))])


# ------------------------------------------------------------------------------------------------------------------ AdamW + EMA
@pytest.mark.parametrize("case", ADAM_CASES, ids=_id)
def test_adamw_ema_step(case):
    table, nulls, n_ema, step, wd, gkind = case
    name = _id(case)
    lay = orf.layout(table, nulls)
    hp = orf.hparams(1e-3, wd, step, n_ema)
    p, g, m, v, e = orf.adam_inputs(lay, step, gkind, seed=step + n_ema)
    P, G, M, V = Arena(lay, p), Arena(lay, g), Arena(lay, m), Arena(lay, v)
    E = [Arena(lay, e[k] if k < n_ema else None) for k in range(4)]
    tab = Tables(lay, P, G, M, V, E)
    chp = c_hparams(hp)

    def call():
        check(lib().mh_adamw_ema_step(tab.tensors.data_ptr(), tab.chunks.data_ptr(), tab.n, C.byref(chp), current_stream()), "mh_adamw_ema_step")
    assert tc.keys_of(call) == [tc.adam_key(n_ema)]
    got_p, got_m, got_v = P.read(name + " p"), M.read(name + " m"), V.read(name + " v")
    G.read(name + " gradient", g)
    got_e = [E[k].read(name + " ema %d" % k, None if k < n_ema else np.full(lay.n, np.nan, F)) for k in range(4)]
    worst, share, fails = orf.judge_adam(lay, (p, g, m, v, e), hp, got_p, got_m, got_v, got_e[:n_ema])
    print("OPTIM-MATRIX adamw %s %s p_bit_equal %.6f" % (name, " ".join("%s %.3f" % kv for kv in worst.items()), share))
    assert not fails, name + ":\n  " + "\n  ".join(fails)
    # a repeated call from the same state gives the same bits
    for a in (P, M, V, *E[:n_ema]):
        a.reset()
    call()
    exact(name, "p repeated", P.read(name), got_p)
    exact(name, "m repeated", M.read(name), got_m)
    exact(name, "v repeated", V.read(name), got_v)
    for k in range(n_ema):
        exact(name, "ema %d repeated" % k, E[k].read(name), got_e[k])


@pytest.mark.parametrize("n_ema", [5, -1])
def test_adamw_ema_step_refuses_an_n_ema_outside_0_to_4(n_ema):
    lay = orf.layout("n63", "first")
    hp = orf.hparams(1e-3, 0.01, 2, 4)
    p, g, m, v, e = orf.adam_inputs(lay, 2, "s1", seed=5)
    P, G, M, V = Arena(lay, p), Arena(lay, g), Arena(lay, m), Arena(lay, v)
    E = [Arena(lay, e[k]) for k in range(4)]
    tab = Tables(lay, P, G, M, V, E)
    chp = c_hparams(hp)
    chp.n_ema = n_ema
    assert lib().mh_adamw_ema_step(tab.tensors.data_ptr(), tab.chunks.data_ptr(), tab.n, C.byref(chp), current_stream()) != 0
    assert lib().mh_last_error()
    torch.cuda.synchronize()
    for a, flat in ((P, p), (G, g), (M, m), (V, v), *zip(E, e)):
        a.read("refused call", flat)


# ------------------------------------------------------------------------------------------------------------------ gradient norm
def _norm_setup(lay, g):
    nan = Arena(lay)            # parameter, moments and EMA copies: the norm and the clip read none of them
    G = Arena(lay, g)
    tab = Tables(lay, nan, G, nan, nan, [nan] * 4)
    return nan, G, tab


def _grad_norm(tab, partial, out):
    check(lib().mh_grad_norm(tab.tensors.data_ptr(), tab.chunks.data_ptr(), tab.n, partial.data_ptr(), out.data_ptr(), current_stream()), "mh_grad_norm")


@pytest.mark.parametrize("case", NORM_CASES, ids=_id)
def test_grad_norm(case):
    table, nulls, gkind = case
    name = _id(case)
    lay = orf.layout(table, nulls)
    g = orf.norm_inputs(lay, gkind, seed=len(lay.chunks))
    nan, G, tab = _norm_setup(lay, g)
    partial, out = nans(tab.n), nans(1)
    assert tc.keys_of(lambda: _grad_norm(tab, partial, out)) == ["sumsq_chunks_kernel", "sum_partials_kernel"]
    got_part, got_norm = read(partial, tab.n, name + " partial"), read(out, 1, name + " out")[0]
    G.read(name + " gradient", g)
    nan.read(name + " other buffers", np.full(lay.n, np.nan, F))
    wp, wn, fails = orf.judge_norm(lay, g, got_part, got_norm)
    if gkind in ("nan", "inf"):
        assert (np.isnan(got_norm) if gkind == "nan" else np.isposinf(got_norm)) and (~np.isfinite(got_part)).sum() == 1
    print("OPTIM-MATRIX norm %s partial %.3f norm %.3f depth %d value %.9g partial_bit_equal %.6f norm_bit_equal %d" % (
        name, wp, wn, orf.total_depth(lay), got_norm, float(orf.same_bits(got_part, orf.sumsq_restate(lay, g)).mean()),
        int(orf.same_bits(orf.norm_restate(got_part), got_norm).all())))
    assert not fails, name + ":\n  " + "\n  ".join(fails)
    partial.fill_(float("nan"))
    out.fill_(float("nan"))
    _grad_norm(tab, partial, out)
    exact(name, "partial repeated", read(partial, tab.n, name), got_part)
    exact(name, "norm repeated", read(out, 1, name), np.array([got_norm], F))


# ------------------------------------------------------------------------------------------------------------------ clip
def _clip(tab, norm, max_norm):
    return lib().mh_clip_grads(tab.tensors.data_ptr(), tab.chunks.data_ptr(), tab.n, norm.data_ptr(), C.c_float(max_norm), current_stream())


def clip_max_norm(mode, norm):
    """the max_norm of a clip case, from the float32 norm the norm kernel wrote"""
    norm = F(norm)
    if mode == "below":
        return F(2) * norm
    if mode == "equal":
        return norm + orf.CLIP_EPS
    if mode == "just_below":
        return np.nextafter(norm + orf.CLIP_EPS, F(0))
    return F(0.5) * norm if np.isfinite(norm) else F(0.5)


@pytest.mark.parametrize("case", CLIP_CASES, ids=_id)
def test_clip_grads(case):
    table, nulls, gkind, mode = case
    name = _id(case)
    lay = orf.layout(table, nulls)
    g = orf.norm_inputs(lay, gkind, seed=len(lay.chunks))
    nan, G, tab = _norm_setup(lay, g)
    partial, out = nans(tab.n), nans(1)
    _grad_norm(tab, partial, out)
    norm = read(out, 1, name + " out")[0]
    max_norm = clip_max_norm(mode, norm)
    assert tc.keys_of(lambda: check(_clip(tab, out, float(max_norm)), "mh_clip_grads")) == ["clip_grads_kernel"]
    want, coef = orf.clip_restate(lay, g, norm, max_norm)
    if mode in ("below", "equal"):
        assert coef == 1.0 and orf.same_bits(want, g).all()
    elif gkind == "inf":
        # an infinite norm: coef = 0, g 0 = 0 (with g's sign) and inf 0 = NaN
        assert np.isposinf(norm) and coef == 0.0 and np.isnan(want[lay.live]).sum() == 1 and (want[lay.live & np.isfinite(g)] == 0).all()
    elif gkind == "nan":
        # a NaN norm: every gradient becomes NaN, as torch.nn.utils.clip_grad_norm_ leaves them
        assert np.isnan(norm) and np.isnan(coef) and np.isnan(want[lay.live]).all()
    else:
        assert 0.0 < coef < 1.0
        if mode == "just_below":
            assert coef >= 1.0 - 4 * orf.U
    got = G.read(name + " gradient")
    _, fails = orf.judge_clip(lay, g, norm, max_norm, got)
    assert not fails, name + ":\n  " + "\n  ".join(fails)
    nan.read(name + " other buffers", np.full(lay.n, np.nan, F))
    exact(name, "norm after the clip", read(out, 1, name), np.array([norm], F))
    read(partial, tab.n, name + " partial")
    print("OPTIM-MATRIX clip %s norm %.9g max_norm %.9g coef %.9g changed %d of %d" % (name, norm, max_norm, coef, int((~orf.same_bits(got, g)).sum()),
                                                                                     int(lay.live.sum())))


@pytest.mark.parametrize("max_norm", [0.0, -1.0])
def test_clip_grads_refuses_a_max_norm_that_is_not_positive(max_norm):
    lay = orf.layout("n63", "first")
    g = orf.norm_inputs(lay, "s1", seed=1)
    nan, G, tab = _norm_setup(lay, g)
    out = nans(1)
    out[0] = 1e3
    assert _clip(tab, out, max_norm) != 0
    assert lib().mh_last_error()
    torch.cuda.synchronize()
    G.read("refused clip", g)


# ------------------------------------------------------------------------------------------------------------------ through the host class
def test_host_class_passes_the_headers_hyper_parameters_and_a_partition():
    """FusedAdamWEMA.step: the mh_opt_hparams the kernel receives (read from the struct at the call) equals float32 of the double-precision
    expressions of include/musehip.h at steps 1, 2, 3 and 100000 with an annealed lr; one-element tensors updated by the kernel with them
    match the restatement; the chunk table read back from the device covers every element of every tensor exactly once at offsets that are
    multiples of 4"""
    from musediffusion_amd import optim
    sizes = (1, 1, 70001, 65536, 5)
    r = np.random.default_rng(0)
    params = [torch.nn.Parameter(torch.from_numpy(r.standard_normal(n).astype(F)).to(DEV)) for n in sizes]
    rates = (0.5, 0.9, 0.99, 0.9999)
    wd = 0.01
    opt = optim.FusedAdamWEMA(params, lr=1e-3, weight_decay=wd, ema_rates=rates)
    ch = opt._chunks.cpu().numpy().view(CHUNK_DTYPE)
    assert len(ch) == opt.n_chunks
    cover = [np.zeros(n, dtype=np.int64) for n in sizes]
    for t, c, o in ch.tolist():
        assert o % 4 == 0 and c > 0 and o + c <= sizes[t]
        cover[t][o:o + c] += 1
    assert all((c == 1).all() for c in cover)
    seen = []
    real = optim.lib()

    class Spy:
        def __getattr__(self, k):
            return getattr(real, k)

        def mh_adamw_ema_step(self, tensors, chunks, n, hp, stream):
            s = hp._obj
            seen.append({k: F(getattr(s, k)) for k in ("beta1", "beta2", "eps", "one_minus_beta1", "one_minus_beta2", "decay_mul", "step_size",
                                                       "bias2_sqrt")} | {"n_ema": s.n_ema, "ema_rate": [F(x) for x in s.ema_rate],
                                                                         "ema_one_minus": [F(x) for x in s.ema_one_minus]})
            return real.mh_adamw_ema_step(tensors, chunks, n, hp, stream)
    spy = Spy()
    old = optim.lib
    optim.lib = lambda: spy
    try:
        for step, lr in ((1, 1e-3), (2, 9e-4), (3, 8e-4), (100000, 1e-4)):
            if step == 100000:
                sd = opt.state_dict()
                for st in sd["state"].values():
                    st["step"] = torch.tensor(99999.0)
                opt.load_state_dict(sd)
            before = [(p.detach().cpu().numpy().copy(), m.cpu().numpy().copy(), v.cpu().numpy().copy()) for p, m, v in zip(params, opt.exp_avg, opt.exp_avg_sq)]
            grads = [r.standard_normal(n).astype(F) for n in sizes]
            for p, gr in zip(params, grads):
                p.grad = torch.from_numpy(gr).to(DEV)
            opt.step(lr=lr)
            want = orf.hparams(lr, wd, step, 4)
            got = seen[-1]
            assert got == want, (step, got, want)
            for i in (0, 1):
                rp, rm, rv = orf.adamw_restate(*before[i][:1], grads[i], *before[i][1:], want)
                assert orf.same_bits(opt.exp_avg[i].cpu().numpy(), rm).all() and orf.same_bits(opt.exp_avg_sq[i].cpu().numpy(), rv).all()
                ref = orf.adamw_ref(before[i][0], grads[i], before[i][1], before[i][2], want)
                assert orf.ratio(params[i].detach().cpu().numpy(), *ref["p"]) <= 1.0
    finally:
        optim.lib = old
    assert len(seen) == 4
