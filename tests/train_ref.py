"""float64 references and per-element error bounds of the training kernels (csrc/train.hip), for tests/test_train_matrix_gpu.py (the
kernels against them) and tests/test_train_bound_cpu.py (a float32 restatement of each reduction kernel stays within half of them).
Imported by test modules; not a conftest.  numpy only, plus torch's erf (numpy has none).

Every reference takes inputs that are already rounded to their storage type (`q`), computes in float64 and returns `(ref, bound)` pairs:
the test is |got - ref| <= bound, element by element.  A bound is first-order forward error analysis of the kernel's own formula, with
u = 2^-24 (one fp32 rounding, relative):

* output rounding: RTOL[dtype] |ref| - 2^-8 for bf16, 2^-22 for fp32, as in the GEMM matrix (tests/test_gemm_matrix_gpu.py);
* an fp32 sum of n terms, in ANY order: n u sum |terms| over the terms actually summed (`sum_err`) - the kernels' wave reductions, 4-lane
  block folds and the 16-lane partial fold all fall under it, so does numpy's pairwise order;
* an error that enters a later formula is carried through it with the formula's own derivative.  The LayerNorm backward is the case that
  matters: dx = rstd (dy g - s1 - xhat s2) is a cancelling difference, so its bound is rstd (|dy g| + |s1| + |xhat| |s2|) times the
  roundings of that line, plus the errors of mean, rstd, xhat, s1 and s2 carried into it - not a multiple of |dx|;
* device tanhf / erff / expf / logf are not bit-reproducible on the host: MATH_ULP units in the last place of their result (the HIP
  math library documents 1 - 2 ulp for these four, numpy's vectorised float32 exp up to 2.6; 8 keeps both within half of the
  allowance), plus the error of the rounded argument times the function's derivative.  exp results below FLT_MIN may be flushed to zero: FLT_MIN absolute.

Nothing here was fitted to what a kernel returned."""
import numpy as np

F32, BF16 = 0, 1
U = 2.0 ** -24
RTOL = {BF16: 2.0 ** -8, F32: 2.0 ** -22}
MATH_ULP = 8.0
FLT_MIN = 2.0 ** -126
ACT_NONE, ACT_TANH, ACT_GELU, ACT_SILU = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------------ storage types
def bf16_round(x):
    """float32 array -> nearest bf16 (ties to even), returned as float32"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


def q(x, dtype):
    """round to the storage type; float32 array holding the stored values"""
    x = np.asarray(x, dtype=np.float32)
    return bf16_round(x) if dtype == BF16 else x


def erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def sum_err(n, abs_terms_sum):
    """an fp32 sum of n terms in any order: at most n u sum |terms|"""
    return n * U * abs_terms_sum


def ratio(got, ref, bound):
    """worst |got - ref| / bound (0 / 0 counts as 0: an exact zero that is exactly zero)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng(seed):
    return np.random.default_rng(seed)


def ln_inputs(rows, H, dtype, seed):
    """x with a per-row offset (|mean| up to 3) and a per-row scale over 100x (rstd varies by 100x across rows); dy ~ N(0, 1) with a
    per-column gain; gamma around 1"""
    g = rng(seed)
    off = g.uniform(-3, 3, (rows, 1))
    scale = 10.0 ** g.uniform(-1.5, 0.5, (rows, 1))
    x = q(off + scale * g.standard_normal((rows, H)), dtype)
    dy = q(g.standard_normal((rows, H)) * (0.5 + g.uniform(0, 1, (1, H))), dtype)
    gamma = (1.0 + 0.3 * g.standard_normal(H)).astype(np.float32)
    return x, dy, gamma


def ln_case_inputs(H, rows, P, acc, dtype):
    """the inputs of a LayerNorm case of the matrix: x, dy, gamma and (accumulate) what dgamma / dbeta hold before the call"""
    x, dy, gamma = ln_inputs(rows, H, dtype, seed=H * 7 + rows)
    g = rng(H + P)
    start_g = g.standard_normal(H).astype(np.float32) * 3 if acc else None
    start_b = g.standard_normal(H).astype(np.float32) * 3 if acc else None
    return x, dy, gamma, start_g, start_b


def colsum_inputs(cols, ld, rows, P, batch, acc, dtype):
    """-> flat (the whole allocation: pitch columns and the gap between batches hold numbers too), stride, x [batch, rows, cols], start"""
    vec = 8 if dtype == BF16 else 4
    stride = rows * ld + (2 * vec if batch > 1 else 0)
    g = rng(cols * 31 + rows + P)
    flat = q(g.standard_normal(batch * stride) + 0.25, dtype)
    x = np.stack([flat[b * stride:b * stride + rows * ld].reshape(rows, ld)[:, :cols] for b in range(batch)])
    start = g.standard_normal((batch, cols)).astype(np.float32) * 5 if acc else None
    return flat, stride, x, start


def scatter_inputs(n, E, V, clamp):
    """ids with one id a third of all tokens (the padding share) and several ids that never occur; clamp: some -1 and V among them"""
    g = rng(n + E)
    live = np.arange(0, V, 3) if V > 8 else np.arange(V - 2)            # ids outside `live` never occur
    ids = g.choice(live, n).astype(np.int32)
    ids[::3] = live[len(live) // 2]
    if clamp:
        ids[5::50], ids[7::50] = -1, V                                  # clamped to 0 and V - 1 by the kernel
    src = g.standard_normal((n, E)).astype(np.float32)
    table = g.standard_normal((V, E)).astype(np.float32)
    return src, ids, table


def ce_inputs(n, V):
    """logits with a per-row shift of +-80; targets include V - 1, 0 and the clamped -1 and V"""
    g = rng(V + n)
    logits = (3 * g.standard_normal((n, V)) + g.choice([-80.0, 80.0], (n, 1))).astype(np.float32)
    target = g.integers(0, V, n).astype(np.int32)
    target[:4] = np.array([V - 1, 0, -1, V], dtype=np.int32)[:n]
    gs = (rng(n).standard_normal(n) * 2).astype(np.float32)
    return logits, target, gs


def sqdiff_inputs(per_batch, B, with_b):
    g = rng(per_batch + B)
    a = (g.standard_normal((B, per_batch)) + 0.5).astype(np.float32)
    b = g.standard_normal((B, per_batch)).astype(np.float32) if with_b else None
    return a, b


def softmax_inputs(L, rows, scale, dtype):
    """scores with one dominant entry (+60 after scaling) in one row; dp for the backward"""
    g = rng(L + rows)
    s = q(4 * g.standard_normal((rows, L)), dtype)
    s[rows // 2, L // 2] = q(np.float32([60.0 / scale]), dtype)[0]
    dp = q(g.standard_normal((rows, L)) * 2, dtype)
    return s, dp


# ------------------------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd(x, dy, gamma, eps, dtype, start_g=None, start_b=None):
    """-> {"dx": (ref, bound), "dgamma": ..., "dbeta": ...}; start_*: what dgamma / dbeta held before an accumulate = 1 call"""
    x, dy, gm = x.astype(np.float64), dy.astype(np.float64), gamma.astype(np.float64)
    rows, H = x.shape
    eps = float(np.float32(eps))
    mean = x.mean(1, keepdims=True)
    e_mean = (H + 1) * U * np.abs(x).mean(1, keepdims=True)
    d = x - mean
    e_d = e_mean + U * np.abs(d)
    var = (d * d).mean(1, keepdims=True)
    e_var = (2 * np.abs(d) * e_d + U * d * d).mean(1, keepdims=True) + (H + 1) * U * var
    rstd = 1.0 / np.sqrt(var + eps)
    r_rstd = 0.5 * (e_var + U * (var + eps)) / (var + eps) + 3 * U          # relative (sqrt, divide, the sum's rounding)
    xh = d * rstd
    e_xh = rstd * e_d + np.abs(xh) * (r_rstd + U)
    dg = dy * gm
    a_dg = np.abs(dg)
    s1 = dg.mean(1, keepdims=True)
    e_s1 = (H + 2) * U * a_dg.mean(1, keepdims=True)
    s2 = (dg * xh).mean(1, keepdims=True)
    e_s2 = (H + 3) * U * (a_dg * np.abs(xh)).mean(1, keepdims=True) + (a_dg * e_xh).mean(1, keepdims=True)
    dx = rstd * (dg - s1 - xh * s2)
    mag = a_dg + np.abs(s1) + np.abs(xh * s2)
    e_dx = rstd * (U * a_dg + e_s1 + np.abs(xh) * e_s2 + np.abs(s2) * e_xh + 3 * U * mag) + (r_rstd + U) * rstd * mag
    out = {"dx": (dx, e_dx + RTOL[dtype] * np.abs(dx)), "dx_arith": e_dx}
    for name, terms, e_terms, start in (("dgamma", dy * xh, np.abs(dy) * e_xh + U * np.abs(dy * xh), start_g), ("dbeta", dy, 0.0 * dy, start_b)):
        ref, a = terms.sum(0), np.abs(terms).sum(0)
        n = rows + 1
        if start is not None:
            ref, a, n = ref + start.astype(np.float64), a + np.abs(start), n + 1
        out[name] = (ref, sum_err(n, a) + e_terms.sum(0) + RTOL[F32] * np.abs(ref))
    return out


def ln_dropped(dx_ref, e_dx, keep, p, dtype):
    """the second output: keep o T(dx) / (1 - p), of the ROUNDED dx as the kernel documents.  The kernel rounds its OWN dx: an error within
    dx's arithmetic bound can flip that rounding to the neighbour, a whole unit in the last place = up to 2 RTOL |dx| just above a power of
    two; then the product is rounded once more"""
    rs = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0
    stored = q(dx_ref, dtype).astype(np.float64)
    ref = np.where(keep, stored * rs, 0.0)
    bound = np.where(keep, (e_dx + 2 * RTOL[dtype] * np.abs(dx_ref)) * rs + RTOL[dtype] * np.abs(ref), 0.0)
    return ref, bound


def ln_bwd_emulate(x, dy, gamma, eps, dtype):
    """ln_bwd_kernel's arithmetic in float32 (formula order the kernel's, summation order numpy's); dx before its rounding to the storage type"""
    f = np.float32
    x, dy, gm = x.astype(f), dy.astype(f), gamma.astype(f)
    H = f(x.shape[1])
    mean = x.sum(1, keepdims=True, dtype=f) / H
    d = x - mean
    rstd = f(1.0) / np.sqrt((d * d).sum(1, keepdims=True, dtype=f) / H + f(eps))
    xh = d * rstd
    dg = dy * gm
    s1 = dg.sum(1, keepdims=True, dtype=f) / H
    s2 = (dg * xh).sum(1, keepdims=True, dtype=f) / H
    dx = rstd * (dg - s1 - xh * s2)
    return dx, (dy * xh).sum(0, dtype=f), dy.sum(0, dtype=f)


# ------------------------------------------------------------------------------------------------------------------ column sums
def col_sum(x, start=None):
    """x [batch, rows, cols] (stored values) -> out [batch, cols]"""
    x = x.astype(np.float64)
    ref, a, n = x.sum(1), np.abs(x).sum(1), x.shape[1]
    if start is not None:
        ref, a, n = ref + start, a + np.abs(start), n + 1
    return ref, sum_err(n, a) + RTOL[F32] * np.abs(ref)


def scatter_add_rows(src, ids, table, V):
    """table[v] + sum of the rows src[t] with clamp(ids[t]) == v"""
    ids = np.clip(ids, 0, V - 1)
    ref, a = table.astype(np.float64).copy(), np.abs(table).astype(np.float64)
    np.add.at(ref, ids, src.astype(np.float64))
    np.add.at(a, ids, np.abs(src).astype(np.float64))
    n = np.bincount(ids, minlength=V).astype(np.float64)[:, None] + 1
    return ref, sum_err(n, a) + RTOL[F32] * np.abs(ref)


# ------------------------------------------------------------------------------------------------------------------ cross-entropy
def _exp_err(e, z):
    """absolute error of expf(z) for a z that carries one rounding of its own (u |z|)"""
    return e * (MATH_ULP + np.abs(z)) * U + FLT_MIN


def ce_fwd(logits, target, V):
    """logits [n, V] (fp32 values) -> {"lse", "loss"}"""
    p = logits.astype(np.float64)
    t = np.clip(target, 0, V - 1)
    mx = p.max(1, keepdims=True)
    z = p - mx
    e = np.exp(z)
    S = e.sum(1, keepdims=True)
    e_S = (_exp_err(e, z)).sum(1, keepdims=True) + sum_err(V, S)
    lse = (mx + np.log(S))[:, 0]
    e_lse = (e_S / S + U + MATH_ULP * U * np.abs(np.log(S)))[:, 0] + U * np.abs(lse)
    loss = lse - p[np.arange(p.shape[0]), t]
    return {"lse": (lse, e_lse + RTOL[F32] * np.abs(lse)), "loss": (loss, e_lse + U * np.abs(loss) + RTOL[F32] * np.abs(loss))}


def ce_fwd_emulate(logits, target, V):
    f = np.float32
    p = logits.astype(f)
    t = np.clip(target, 0, V - 1)
    mx = p.max(1, keepdims=True)
    S = np.exp(p - mx).sum(1, keepdims=True, dtype=f)
    lse = (mx + np.log(S))[:, 0]
    return lse, lse - p[np.arange(p.shape[0]), t]


def ce_bwd(logits, target, lse, g, V, dtype):
    """(exp(logit - lse) - onehot) g, with lse and g the fp32 values the kernel is given"""
    p = logits.astype(np.float64)
    t = np.clip(target, 0, V - 1)
    z = p - lse.astype(np.float64)[:, None]
    e = np.exp(z)
    oh = np.zeros_like(p)
    oh[np.arange(p.shape[0]), t] = 1.0
    gs = g.astype(np.float64)[:, None]
    ref = (e - oh) * gs
    bound = np.abs(gs) * (_exp_err(e, z) + U * np.abs(e - oh)) + U * np.abs(ref) + RTOL[dtype] * np.abs(ref)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------ squared error
def _sqdiff_d(a, b, scale_a):
    sa = float(np.float32(scale_a))
    a = a.astype(np.float64)
    bb = 0.0 if b is None else b.astype(np.float64)
    d = sa * a - bb
    return sa, d, U * (np.abs(sa * a) + np.abs(d))


def sqdiff_mean(a, b, scale_a):
    """a, b [B, per_batch] -> out [B]"""
    _, d, e_d = _sqdiff_d(a, b, scale_a)
    n = d.shape[1]
    ref = (d * d).mean(1)
    return ref, (2 * np.abs(d) * e_d + U * d * d).mean(1) + sum_err(n + 1, ref) + RTOL[F32] * ref


def sqdiff_mean_emulate(a, b, scale_a):
    f = np.float32
    d = f(scale_a) * a.astype(f) - (f(0) if b is None else b.astype(f))
    return (d * d).sum(1, dtype=f) / f(d.shape[1])


def sqdiff_bwd(a, b, scale_a, g, start_a=None, start_b=None):
    """-> {"da", "db"}: da = start + g 2 scale_a (scale_a a - b) / per_batch, db = start - g 2 (scale_a a - b) / per_batch"""
    sa, d, e_d = _sqdiff_d(a, b, scale_a)
    n = d.shape[1]
    gs = g.astype(np.float64)[:, None]
    base = gs * 2.0 * d / n
    e_base = np.abs(gs) * 2.0 * e_d / n + 3 * U * np.abs(base)
    out = {}
    for name, v, e_v, start in (("da", base * sa, e_base * abs(sa) + U * np.abs(base * sa), start_a), ("db", -base, e_base, start_b)):
        ref = v if start is None else start.astype(np.float64) + v
        out[name] = (ref, e_v + U * np.abs(ref) + RTOL[F32] * np.abs(ref))
    return out


def scale_rows(src, scale, mask, E, start=None):
    """src [B, per_batch]; mask per token (E elements each, flat over the batch), 0 = anchored (factor 1)"""
    B, n = src.shape
    mult = np.ones((B, n)) if scale is None else np.repeat(scale.astype(np.float64)[:, None], n, 1)
    if mask is not None:
        anchored = np.repeat(mask == 0, E)[:B * n].reshape(B, n)
        mult = np.where(anchored, 1.0, mult)
    v = src.astype(np.float64) * mult
    ref = v if start is None else start.astype(np.float64) + v
    return ref, U * (np.abs(v) + np.abs(ref)) + RTOL[F32] * np.abs(ref)


# ------------------------------------------------------------------------------------------------------------------ row softmax
def softmax_rows(s, scale, dtype):
    """s [rows, L] stored scores -> softmax(s scale) in the storage type"""
    sc = float(np.float32(scale))
    t = s.astype(np.float64) * sc
    mx = t.max(1, keepdims=True)
    z = t - mx
    e_z = U * (np.abs(t) + np.abs(mx))          # t and mx carry the rounding of the product; the difference one more (in _exp_err)
    e = np.exp(z)
    e_e = _exp_err(e, z) + e * e_z
    S = e.sum(1, keepdims=True)
    r_S = (e_e.sum(1, keepdims=True) + sum_err(s.shape[1], S)) / S
    ref = e / S
    return ref, e_e / S + ref * (r_S + 3 * U) + RTOL[dtype] * ref


def softmax_rows_emulate(s, scale, dtype):
    f = np.float32
    t = s.astype(f) * f(scale)
    e = np.exp(t - t.max(1, keepdims=True))
    return e * (f(1.0) / e.sum(1, keepdims=True, dtype=f))


def softmax_bwd_rows(p, dp, scale, dtype):
    """p (dp - sum(dp p)) scale"""
    sc = float(np.float32(scale))
    p, dp = p.astype(np.float64), dp.astype(np.float64)
    L = p.shape[1]
    dot = (p * dp).sum(1, keepdims=True)
    e_dot = sum_err(L + 1, np.abs(p * dp).sum(1, keepdims=True))
    ref = p * (dp - dot) * sc
    bound = np.abs(p * sc) * (e_dot + U * (np.abs(dp) + np.abs(dot))) + 2 * U * np.abs(ref) + RTOL[dtype] * np.abs(ref)
    return ref, bound


def softmax_bwd_rows_emulate(p, dp, scale, dtype):
    f = np.float32
    p, dp = p.astype(f), dp.astype(f)
    dot = (p * dp).sum(1, keepdims=True, dtype=f)
    return p * (dp - dot) * f(scale)


# ------------------------------------------------------------------------------------------------------------------ activations
K_ERF = 0.70710678118654752440
K_PDF = 0.3989422804014327


def _erf_err(x):
    """absolute error of erff(x K_ERF): MATH_ULP ulp of the result + the argument's rounding times erf'"""
    a = x * K_ERF
    return MATH_ULP * U * np.abs(erf(a)) + 2.0 / np.sqrt(np.pi) * np.exp(-a * a) * U * np.abs(a)


def act_fwd(x, act, dtype):
    x = x.astype(np.float64)
    if act == ACT_TANH:
        ref = np.tanh(x)
        e = MATH_ULP * U * np.abs(ref)
    elif act == ACT_GELU:
        one = 1.0 + erf(x * K_ERF)
        ref = 0.5 * x * one
        e = 0.5 * np.abs(x) * (_erf_err(x) + U * np.abs(one)) + 2 * U * np.abs(ref)
    elif act == ACT_SILU:
        en = np.exp(-x)
        ref = x / (1.0 + en)
        e = np.abs(ref) * (en / (1.0 + en) * MATH_ULP * U + 2 * U)
    else:
        ref, e = x, 0.0 * x
    return ref, e + RTOL[dtype] * np.abs(ref)


def act_deriv(x, act):
    """act'(x) and the absolute error of the kernel's fp32 formula for it"""
    if act == ACT_TANH:
        t = np.tanh(x)
        d = 1.0 - t * t
        return d, 2 * np.abs(t) * MATH_ULP * U * np.abs(t) + U * t * t + U * np.abs(d)
    if act == ACT_GELU:
        one = 1.0 + erf(x * K_ERF)
        a = -0.5 * x * x
        t2 = x * K_PDF * np.exp(a)
        d = 0.5 * one + t2
        e = 0.5 * (_erf_err(x) + U * np.abs(one)) + np.abs(t2) * (MATH_ULP + 2 * np.abs(a) + 3) * U + FLT_MIN * np.abs(x) + U * np.abs(d)
        return d, e
    if act == ACT_SILU:
        en = np.exp(-x)
        sg = 1.0 / (1.0 + en)
        e_sg = sg * (en * sg * MATH_ULP + 2) * U
        om = 1.0 - sg
        e_om = e_sg + U * np.abs(om)
        inner = 1.0 + x * om
        e_in = np.abs(x) * e_om + U * np.abs(x * om) + U * np.abs(inner)
        d = sg * inner
        return d, np.abs(inner) * e_sg + sg * e_in + U * np.abs(d)
    return np.ones_like(x), 0.0 * x


def act_bwd(dy, x, act, dtype):
    x, g = x.astype(np.float64), dy.astype(np.float64)
    d, e_d = act_deriv(x, act)
    ref = g * d
    return ref, np.abs(g) * e_d + U * np.abs(ref) + RTOL[dtype] * np.abs(ref)


def act_emulate(x, act, dy=None):
    """the kernels' fp32 formulas with numpy's float32 functions (torch's for erf); forward, or dy act'(x)"""
    import torch
    f = np.float32
    x = x.astype(f)
    erf32 = lambda v: torch.erf(torch.from_numpy(np.ascontiguousarray(v, dtype=f))).numpy()
    if dy is None:
        if act == ACT_TANH:
            return np.tanh(x)
        if act == ACT_GELU:
            return f(0.5) * x * (f(1.0) + erf32(x * f(K_ERF)))
        if act == ACT_SILU:
            return x / (f(1.0) + np.exp(-x))
        return x
    d = np.ones_like(x)
    if act == ACT_TANH:
        t = np.tanh(x)
        d = f(1.0) - t * t
    elif act == ACT_GELU:
        d = f(0.5) * (f(1.0) + erf32(x * f(K_ERF))) + x * f(K_PDF) * np.exp(f(-0.5) * x * x)
    elif act == ACT_SILU:
        sg = f(1.0) / (f(1.0) + np.exp(-x))
        d = sg * (f(1.0) + x * (f(1.0) - sg))
    return dy.astype(f) * d


def act_inputs(n, dtype, seed):
    """[-12, 12] with exact zeros and the end points"""
    x = rng(seed).uniform(-12, 12, n).astype(np.float32)
    x[::97] = 0.0
    x[0] = 0.0 if n == 1 else -12.0
    x[-1] = 0.0 if n == 1 else 12.0
    if n > 8:
        x[1:8] = (-0.0, 1e-3, -1e-3, 0.5, -0.5, 3.0, -3.0)
    return q(x, dtype)


# ------------------------------------------------------------------------------------------------------------------ exact kernels
def add_pos_time(x, pos, emb, dtype):
    """(pos[l] + x[b, l]) + emb[b] in float32, rounded once: bit for bit what the kernel stores.  x [B, L, H]"""
    f = np.float32
    return q((pos.astype(f)[None] + x.astype(f)) + emb.astype(f)[:, None, :], dtype)


def add_inplace(dst, src, dtype):
    return q(dst.astype(np.float32) + src.astype(np.float32), dtype)


def perm16(L):
    """mode 3 / 4 of mh_head_permute: within every group of 16 positions the stored order is 0-3, 8-11, 4-7, 12-15"""
    l = np.arange(L)
    return (l & ~15) | ((((l >> 3) & 1) | ((l >> 1) & 2)) << 2) | (l & 3)


def head_permute(x, B, L, nh, dh, mode):
    """the documented layouts.  modes 0, 2, 3, 4: x = tokens [B L, nh dh] -> heads [B, nh, L, dh] (0) or [B, nh, dh, L] (2; 3 / 4 with the
    P-operand position order).  mode 1: x = heads [B, nh, L, dh] -> tokens [B L, nh dh]"""
    if mode == 1:
        return x.reshape(B, nh, L, dh).transpose(0, 2, 1, 3).reshape(B * L, nh * dh)
    h = x.reshape(B, L, nh, dh).transpose(0, 2, 1, 3)          # [B, nh, L, dh]
    if mode == 0:
        return np.ascontiguousarray(h)
    if mode >= 3:
        h = h[:, :, perm16(L), :]
    return np.ascontiguousarray(h.transpose(0, 1, 3, 2))


def to_panel(x, ld):
    """[rows, cols] -> K32 panels [cols / 32][ld rows][32]; rows beyond x's are NaN"""
    rows, cols = x.shape
    out = np.full((cols // 32, ld, 32), np.nan, dtype=x.dtype)
    out[:, :rows, :] = x.reshape(rows, cols // 32, 32).transpose(1, 0, 2)
    return out


def from_panel(p, rows):
    """K32 panels [cols / 32][ld][32] -> [rows, cols]"""
    return np.ascontiguousarray(p[:, :rows, :].transpose(1, 0, 2)).reshape(rows, -1)
