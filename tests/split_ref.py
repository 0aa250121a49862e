"""float64 references and per-element error bounds of the split-precision kernels (csrc/split.hip), for tests/test_split_matrix_gpu.py (the
kernels against them) and tests/test_split_bound_cpu.py (a float32 restatement of each kernel with emulated 16-bit parts stays within half
of them, and one with a single injected error leaves them).  Imported by test modules; not a conftest.  numpy only, plus torch's erf.

A split value is a pair (hi, lo) of 16-bit floats, here two float32 arrays that hold exactly representable values.  References are plain
float64 numpy on the STORED operands: fp32 values for pack and layernorm, the exact hi + lo for everything that reads parts.  Every
reference returns `(ref, bound)`; the test is |got - ref| <= bound per element, with got = hi + lo of the stored output parts (exact in
float64).  The terms, each next to the source line it comes from (u = 2^-24, helpers and conventions of tests/train_ref.py and
tests/step_ref.py: a lone rounding counts 2 u, an fp32 sum of n terms in any order n u sum |terms|, a math function MATH_ULP ulp):

* store_split8 / split(): hi = rn16(sat(v)), lo = rn16(v - hi), the difference exact in fp32.  bf16 keeps 8 significant bits: |v - hi| <=
  2^-8 |v| and |rem - lo| <= 2^-8 |rem|, together 2^-16 |v|.  fp16 keeps 11: 2^-22 |v|, and where a part is subnormal (below 2^-14) it is
  a multiple of 2^-24: 2^-25 absolute (`part_err`).  Nothing is allowed for sat(): the matrix keeps fp16 values below 65504 outside the
  pack cases, which compare bit for bit.
* Sp<T>::split2 (the attention probabilities, by truncation): bf16 hi = the top 16 bits, lo = the top 16 bits of the exact remainder; the
  remainder holds the 16 low bits of the fp32 significand and lo keeps the upper 8 of them: 2^-15 |p|.  fp16 (v_cvt_pkrtz): the remainder
  holds 13 bits, lo keeps 11: 2^-21 |p|; below 2^-14 the parts are multiples of 2^-24: min(p, 2^-24) absolute (`trunc_err`).
* the product dropped from every sum, lo x lo: sum |a_lo| |w_lo| of the actual parts (attention P V: |p_lo| <= 2^-7 p / 2^-10 p, the
  truncation remainder, times the actual |v_lo|).
* the MFMA K loops: products of two 16-bit floats are exact in fp32; three products per K element accumulate in fp32, in any order:
  3 K u sum (|a_hi| + |a_lo|) (|w_hi| + |w_lo|), computed exactly as a matrix product of absolute values.
* epilogues: `acc + bv + br` (split.hip: v[e] = acc + bv[e] + br) two roundings; tanhf / erff as tests/train_ref.py: act_fwd states them,
  the error of the argument carried with the derivative; the residual `(float)hv + (float)lv` one rounding, its sum another.
* LayerNorm statistics: tests/step_ref.py: layernorm (two-pass, errors carried from stage to stage) with the longest addition chain of
  each kernel: split_ln_kernel as csrc/norm.hip's row kernel (8 per chunk round + 6 shuffle levels), split_gemm_ln_kernel 32 in-lane
  values + 2 shuffles + the 4 column waves.
* online softmax (split_attn_kernel): p = v_exp_f32(fma(s, c, -m c)) with c = scale log2 e in fp32 (the reference uses the same fp32
  constant); the running sums are rescaled by alpha = v_exp_f32((m_old - m_new) c) once per key tile: ceil(L / 64) factors of relative error
  MATH_ULP u, and ln 2 times the rounding of their arguments, which add up to the rise of the row's running maximum; a final reciprocal
  and product.  Errors of the running maximum itself cancel between numerator and denominator.  Results of v_exp_f32 below FLT_MIN may be
  flushed: FLT_MIN.  The attention's sums follow the kernel's own MFMA order (16 products per instruction, in any order inside it), so
  their term is step_ref.chain_err with the longest chain of additions: 16 + 3 dh / 16 for a score, 16 + 13 per key tile for O.

Nothing here was fitted to what a kernel returned."""
import numpy as np

import step_ref as st
import train_ref as tr
from train_ref import FLT_MIN, MATH_ULP, U, ratio  # noqa: F401  (re-exported for the test modules)

BF16X3, F16X3 = 2, 3          # musediffusion_amd._lib: MH_BF16X3, MH_F16X3
DTYPES = (BF16X3, F16X3)
NAME = {BF16X3: "bf16x3", F16X3: "f16x3"}
F16_MAX = 65504.0
ACT_NONE, ACT_TANH, ACT_GELU = 0, 1, 2
LOG2E_F32 = np.float32(1.4426950408889634)
LN2 = float(np.log(2.0))
f32 = np.float32


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------------------------ 16-bit parts
def rn16(x, dt):
    """float32 -> nearest value of the 16-bit type (ties to even), as float32"""
    x = np.ascontiguousarray(x, dtype=f32)
    if dt == BF16X3:
        return tr.bf16_round(x)
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(f32)


def sat(x, dt):
    """Sp<T>::sat: fminf(fmaxf(v, -65504), 65504) for fp16 parts (a NaN becomes -65504: fmaxf returns the other operand), v for bf16"""
    x = np.asarray(x, dtype=f32)
    if dt == BF16X3:
        return x
    return np.minimum(np.where(np.isnan(x), f32(-F16_MAX), np.maximum(x, f32(-F16_MAX))), f32(F16_MAX)).astype(f32)


def split_rn(v, dt):
    """split(): the stored parts of fp32 values, bit for bit"""
    s = sat(v, dt)
    hi = rn16(s, dt)
    with np.errstate(invalid="ignore"):
        lo = rn16((s - hi).astype(f32), dt)
    return hi, lo


def rtz16(x, dt):
    """float32 -> the 16-bit type rounded toward zero, as float32 (bf16: the top 16 bits; fp16: the nearest, stepped back where it grew)"""
    x = np.ascontiguousarray(x, dtype=f32)
    if dt == BF16X3:
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32).reshape(x.shape)
    h = x.astype(np.float16)
    grew = np.abs(h.astype(f32)) > np.abs(x)
    return np.where(grew, np.nextafter(h, np.float16(0)), h).astype(f32)


def split_trunc(p, dt):
    """Sp<T>::split2: parts by truncation"""
    hi = rtz16(p, dt)
    return hi, rtz16((np.asarray(p, dtype=f32) - hi).astype(f32), dt)


def val(parts):
    """the value a pair of parts stands for, exact in float64"""
    return parts[0].astype(np.float64) + parts[1].astype(np.float64)


def mag(parts):
    return np.abs(parts[0]).astype(np.float64) + np.abs(parts[1]).astype(np.float64)


def part_err(v, dt):
    """|v - (hi + lo)| of store_split8 for an fp32 v (see the module docstring)"""
    v = np.abs(v)
    return 2.0 ** -16 * v if dt == BF16X3 else 2.0 ** -22 * v + 2.0 ** -25


def trunc_err(p, dt):
    p = np.abs(p)
    return 2.0 ** -15 * p if dt == BF16X3 else 2.0 ** -21 * p + np.minimum(p, 2.0 ** -24)


def trunc_lo(dt):
    """|p_lo| <= trunc_lo p: the remainder of the truncated hi part"""
    return 2.0 ** -7 if dt == BF16X3 else 2.0 ** -10


# ------------------------------------------------------------------------------------------------------------------ layouts
def to_panels(parts, ld, kpad=None, fill=np.nan):
    """parts of [rows, cols] -> split panels [2][kpad / 32][ld][32] (float32 values); rows beyond `rows` hold `fill`, the K padding zero"""
    rows, cols = parts[0].shape
    kpad = kpad or (cols + 31) // 32 * 32
    out = np.full((2, kpad // 32, ld, 32), fill, dtype=f32)
    for p in range(2):
        x = np.zeros((rows, kpad), dtype=f32)
        x[:, :cols] = parts[p]
        out[p, :, :rows, :] = x.reshape(rows, kpad // 32, 32).transpose(1, 0, 2)
    return out


def from_panels(pan, rows, cols):
    """split panels [2][npanels][ld][32] -> (hi, lo) [rows, cols]"""
    return tuple(np.ascontiguousarray(pan[p][:, :rows, :].transpose(1, 0, 2)).reshape(rows, -1)[:, :cols] for p in range(2))


# ------------------------------------------------------------------------------------------------------------------ inputs
def pack_inputs(rows, cols, dt, seed):
    """fp32 rows: O(1) values with a column gain, magnitude 1e-3 (subnormal fp16 lo parts), and in the first rows 65504, the value
    above it that still rounds to it, 1e6 and +-inf with both signs"""
    g = rng(seed)
    x = (g.standard_normal((rows, cols)) * np.array([1.0, 30.0, 0.2, 1e-3])[np.arange(cols) % 4]).astype(f32)
    special = np.array([65504.0, -65504.0, 65519.0, 1e6, -1e6, np.inf, -np.inf, 1e-3, 6e-8, 0.0, -0.0], dtype=f32)
    flat = x.reshape(-1)
    n = min(flat.size, special.size)
    flat[:n] = special[:n]
    return x


def values(shape, dt, seed, scale=1.0):
    """a split operand: fp32 draws -> stored parts"""
    return split_rn((rng(seed).standard_normal(shape) * scale).astype(f32), dt)


def ln_inputs(rows, H, seed):
    """fp32 rows with a per-row offset and a per-row scale over 100x; with more than one row, row 0 constant (more than two: the last too) and row 1 with a mean
    1e3 times its spread; gamma around 1, beta around 0"""
    g = rng(seed)
    x = (g.uniform(-3, 3, (rows, 1)) + 10.0 ** g.uniform(-1.5, 0.5, (rows, 1)) * g.standard_normal((rows, H))).astype(f32)
    if rows > 1:
        x[0] = f32(0.75)
        x[1] = (100.0 + 0.1 * g.standard_normal(H)).astype(f32)
    if rows > 2:
        x[-1] = f32(-2.0)
    gamma = (1.0 + 0.3 * g.standard_normal(H)).astype(f32)
    beta = (0.2 * g.standard_normal(H)).astype(f32)
    return x, gamma, beta


# ------------------------------------------------------------------------------------------------------------------ pack / join
def join(parts):
    """split_join_kernel / load_split8: (float)hi + (float)lo in fp32, bit for bit"""
    with np.errstate(invalid="ignore"):
        return (parts[0].astype(f32) + parts[1].astype(f32)).astype(f32)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm(x, pos, emb, rows_of, L, gamma, beta, eps, dt):
    """split_ln_kernel: y = LN((pos[l] + x) + emb[rows_of[b]]) (pos None: LN(x)) -> (ref, bound) of hi + lo"""
    v = x.astype(np.float64)
    e0 = np.zeros_like(v)
    if pos is not None:
        n = x.shape[0]
        l, b = np.arange(n) % L, np.arange(n) // L
        s1 = pos[l].astype(np.float64) + v
        v = s1 + emb[rows_of[b]].astype(np.float64)
        e0 = 2 * U * (np.abs(s1) + np.abs(v))          # v[i][e] = (p[e] + v[i][e]) + t[e]: two roundings
    y, bound = st.layernorm(v, gamma, beta, float(f32(eps)), tr.F32, st.ln_depth(x.shape[1], "rows"), ein=e0)
    return y, bound - tr.RTOL[tr.F32] * np.abs(y) + part_err(y, dt)          # (the output is rounded into parts, not to fp32)


def layernorm_emulate(x, pos, emb, rows_of, L, gamma, beta, eps, dt, unbiased=False):
    """split_ln_kernel in float32 (numpy's summation order) -> stored parts.  unbiased: the injected error (variance over H - 1)"""
    v = x.astype(f32)
    if pos is not None:
        n = x.shape[0]
        l, b = np.arange(n) % L, np.arange(n) // L
        v = ((pos[l].astype(f32) + v).astype(f32) + emb[rows_of[b]].astype(f32)).astype(f32)
    return split_rn(_ln32(v, gamma, beta, eps, unbiased), dt)


def _ln32(v, gamma, beta, eps, unbiased=False):
    H = f32(v.shape[1])
    mean = (v.sum(1, keepdims=True, dtype=f32) / H).astype(f32)
    d = (v - mean).astype(f32)
    var = ((d * d).sum(1, keepdims=True, dtype=f32) / (H - f32(1) if unbiased else H)).astype(f32)
    rstd = (f32(1.0) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)
    return (((d * rstd).astype(f32) * gamma.astype(f32)).astype(f32) + beta.astype(f32)).astype(f32)


# ------------------------------------------------------------------------------------------------------------------ GEMM
def _products(A, W):
    """-> z = a w^T, e_z: the dropped lo x lo product + the fp32 accumulation of 3 K products"""
    a, w = val(A), val(W)
    K = a.shape[1]
    z = a @ w.T
    e_z = np.abs(A[1]).astype(np.float64) @ np.abs(W[1]).astype(np.float64).T + 3 * K * U * (mag(A) @ mag(W).T)
    return z, e_z


def _act(pre, e_pre, act):
    """act(pre) and its error: the function's own (train_ref.act_fwd, without its output rounding) + act' e_pre"""
    if act == ACT_NONE:
        return pre, e_pre
    ref, e = tr.act_fwd(pre, act, tr.F32)
    d, _ = tr.act_deriv(pre, act)
    return ref, e - tr.RTOL[tr.F32] * np.abs(ref) + np.abs(d) * e_pre


def gemm(A, W, bias_col, bias_row, act, R, out_mode, dt):
    """split_gemm_kernel: act(A W^T + bias) [+ residual]; A, W, R pairs of parts; out_mode 2: fp32 rows, else parts -> (ref, bound)"""
    z, e_z = _products(A, W)
    b = np.zeros_like(z)
    if bias_col is not None:
        b = b + bias_col.astype(np.float64)[None, :]
    if bias_row is not None:
        b = b + bias_row.astype(np.float64)[:, None]
    pre = z + b
    e_pre = e_z + 2 * U * (np.abs(z) + np.abs(pre))          # v[e] = acc + bv[e] + br
    ref, e = _act(pre, e_pre, act)
    if R is not None:
        r = val(R)
        e = e + 2 * U * np.abs(r) + 2 * U * np.abs(ref + r)          # load_split8: (float)hv + (float)lv; v[e] += rv[e]
        ref = ref + r
    return ref, e + (part_err(ref, dt) if out_mode != 2 else 0.0) + 1e-300


def gemm_emulate(A, W, bias_col, bias_row, act, R, out_mode, dt, drop=None):
    """split_gemm_kernel in float32 (BLAS summation order).  drop: "lo" (lo parts zeroed), "hilo" (the A hi x W lo product dropped),
    "reslo" (the residual's lo part skipped), "biascol" (bias[col] where bias[row] is meant)"""
    Ah, Al, Wh, Wl = (t.astype(f32) for t in (A[0], A[1], W[0], W[1]))
    if drop == "lo":
        Al, Wl = np.zeros_like(Al), np.zeros_like(Wl)
    acc = Al @ Wh.T
    if drop != "hilo":
        acc = (acc + Ah @ Wl.T).astype(f32)
    acc = (acc + Ah @ Wh.T).astype(f32)
    if bias_col is not None:
        acc = (acc + bias_col.astype(f32)[None, :]).astype(f32)
    if bias_row is not None:
        n = acc.shape[1]
        acc = (acc + (np.resize(bias_row.astype(f32), n)[None, :] if drop == "biascol" else bias_row.astype(f32)[:, None])).astype(f32)
    v = tr.act_emulate(acc, act)
    if R is not None:
        v = (v + (R[0].astype(f32) if drop == "reslo" else join(R))).astype(f32)
    return v if out_mode == 2 else split_rn(v, dt)


GEMM_LN_DEPTH = 32 + 2 + 4          # split_gemm_ln_kernel: a lane's 32 values, two shuffles, the four column waves (+ the mean's own)


def gemm_ln(A, W, bias, R, gamma, beta, eps, dt):
    """split_gemm_ln_kernel: LN(A W^T + bias + residual) as parts"""
    z, e_z = _products(A, W)
    r = val(R)
    s1 = z + bias.astype(np.float64)[None, :]
    pre = s1 + r
    e_pre = e_z + 2 * U * (np.abs(z) + np.abs(s1)) + 2 * U * np.abs(r) + 2 * U * np.abs(pre)          # (acc + bv[e]) + rv[e]
    y, bound = st.layernorm(pre, gamma, beta, float(f32(eps)), tr.F32, GEMM_LN_DEPTH, ein=e_pre)
    return y, bound - tr.RTOL[tr.F32] * np.abs(y) + part_err(y, dt)


def gemm_ln_emulate(A, W, bias, R, gamma, beta, eps, dt, drop=None, unbiased=False):
    pre = gemm_emulate(A, W, bias, None, ACT_NONE, R, 2, dt, drop)
    return split_rn(_ln32(pre, gamma, beta, eps, unbiased), dt)


# ------------------------------------------------------------------------------------------------------------------ attention
def scale_log2e(scale):
    """launch_attn: scale * 1.4426950408889634f in fp32"""
    return f32(f32(scale) * LOG2E_F32)


def _heads(x, B, L, nh, dh):
    return x.reshape(B, L, nh, dh).transpose(0, 2, 1, 3)


def attn_inputs(B, L, nh, dh, profile, dt, seed):
    """q, k, v parts [B L, H].  profile: "plain"; "rising" / "falling": every query carries a constant 2 in its first component and key j
    0.1 j (0.1 (L - 1 - j)) in its, so the scores rise (fall) by 12.8 per key tile against a noise of about sqrt(dh) / 4: every tile (only
    the first) raises the running maximum; "underflow": plain operands, meant for a scale that leaves exp2 nonzero for a few keys only"""
    g = rng(seed)
    H = nh * dh
    q, k, v = (g.standard_normal((B * L, H)) * s for s in (0.5, 0.5, 1.0))
    if profile in ("rising", "falling"):
        j = np.tile(np.arange(L), B).astype(np.float64)
        q[:, ::dh] = 2.0
        k[:, ::dh] = (0.1 * j if profile == "rising" else 0.1 * (L - 1 - j))[:, None]
    return tuple(split_rn(t.astype(f32), dt) for t in (q, k, v))


def attention(q, k, v, B, L, nh, dh, scale, dt):
    """split_attn_kernel: softmax(q k^T scale) v per (batch, head), the exponent constant the kernel's fp32 one -> (ref, bound) [B L, H]"""
    c = float(scale_log2e(scale))
    hd = lambda t: _heads(t, B, L, nh, dh)
    qv, kv, vv = hd(val(q)), hd(val(k)), hd(val(v))
    s = np.einsum("bhid,bhjd->bhij", qv, kv)
    # S^T = K_hi Q_lo^T + K_lo Q_hi^T + K_hi Q_hi^T: the dropped product; 3 dh / 16 MFMAs in the kernel's own order, each the sum of 16
    # products in any order: the longest chain of additions has 16 + 3 dh / 16 links (step_ref.chain_err)
    e_s = np.einsum("bhid,bhjd->bhij", hd(np.abs(q[1]).astype(np.float64)), hd(np.abs(k[1]).astype(np.float64))) + \
        st.chain_err(16 + 3 * dh // 16, np.einsum("bhid,bhjd->bhij", hd(mag(q)), hd(mag(k))))
    m = s.max(-1, keepdims=True)
    arg = (s - m) * c
    w = np.exp2(arg)
    nt = (L + 63) // 64
    # the running maximum's total rise after the first key tile, in exponent units: the alpha arguments of a row add up to it
    rise = (m - s[..., :64].max(-1, keepdims=True)) * abs(c)
    # p = exp2f(fmaf(s, c, -mb)): mb = m_new c one rounding, the fma one
    e_arg = abs(c) * e_s + 2 * U * (abs(c) * np.abs(s).max(-1, keepdims=True) + np.abs(arg))
    # alpha = exp2f((m_run - m_new) c) once per key tile: the function's ulps and the product o *= alpha each time; the two roundings of
    # its argument are relative to the argument, and the arguments of all tiles add up to `rise`
    e_w = w * (MATH_ULP * U + LN2 * e_arg + nt * (MATH_ULP * U + 2 * U) + LN2 * 4 * U * rise) + FLT_MIN
    l = w.sum(-1, keepdims=True)
    e_l = e_w.sum(-1, keepdims=True) + st.chain_err(32 + nt + 1, l)          # psum over a lane's 32 registers, nt rescaled additions, two half-waves
    av, av_lo = hd(mag(v)), hd(np.abs(v[1]).astype(np.float64))
    num = np.einsum("bhij,bhjd->bhid", w, vv)
    # O^T += V^T_hi P_lo^T + V^T_lo P_hi^T + V^T_hi P_hi^T on the truncated parts of p: 12 MFMAs of 16 keys per key tile in the
    # kernel's own order and one rescale: a chain of 16 + 13 nt links
    e_num = np.einsum("bhij,bhjd->bhid", e_w + trunc_err(w, dt), av) + trunc_lo(dt) * np.einsum("bhij,bhjd->bhid", w, av_lo) + \
        st.chain_err(16 + 13 * nt, np.einsum("bhij,bhjd->bhid", w, av))
    o = num / l
    e_o = e_num / l + np.abs(o) * (e_l / l + 4 * U)          # inv = 1.0f / l_tot; o * inv
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(B * L, nh * dh)
    o, e_o = back(o), back(e_o)
    return o, e_o + part_err(o, dt) + 1e-300


def attention_emulate(q, k, v, B, L, nh, dh, scale, dt, drop=None):
    """split_attn_kernel in float32: key tiles of 64, the online softmax with one rescale per tile, truncated probability parts.
    drop: "lo" (lo parts of q, k, v zeroed), "rescale" (the rescale of o skipped on the second tile), "alpha" (alpha from the new maximum
    on both sides: 1), "plo" (the V_hi x P_lo product dropped)"""
    c = scale_log2e(scale)
    hd = lambda t: _heads(t.astype(f32), B, L, nh, dh)
    qh, ql, kh, kl, vh, vl = hd(q[0]), hd(q[1]), hd(k[0]), hd(k[1]), hd(v[0]), hd(v[1])
    if drop == "lo":
        ql, kl, vl = np.zeros_like(ql), np.zeros_like(kl), np.zeros_like(vl)
    mm = lambda a, b: np.einsum("bhid,bhjd->bhij", a, b).astype(f32)
    pv = lambda p, x: np.einsum("bhij,bhjd->bhid", p, x).astype(f32)
    o = np.zeros(qh.shape, dtype=f32)
    m_run = np.full(qh.shape[:3] + (1,), -np.inf, dtype=f32)
    l_run = np.zeros(qh.shape[:3] + (1,), dtype=f32)
    for t in range((L + 63) // 64):
        j = slice(64 * t, min(L, 64 * t + 64))
        s = ((mm(ql, kh[:, :, j]) + mm(qh, kl[:, :, j])).astype(f32) + mm(qh, kh[:, :, j])).astype(f32)
        m_new = np.maximum(m_run, s.max(-1, keepdims=True))
        with np.errstate(invalid="ignore"):
            alpha = np.exp2(((m_run - m_new) * c).astype(f32)).astype(f32)
        alpha = np.where(np.isneginf(m_run), f32(0), alpha)
        if drop == "alpha" and t > 0:
            alpha = np.ones_like(alpha)
        mb = (m_new * c).astype(f32)
        p = np.exp2((s.astype(np.float64) * float(c) - mb).astype(f32)).astype(f32)          # fmaf: one rounding
        l_run = (l_run * alpha + p.sum(-1, keepdims=True, dtype=f32)).astype(f32)
        m_run = m_new
        if not (drop == "rescale" and t == 1):
            o = (o * alpha).astype(f32)
        ph, pl = split_trunc(p, dt)
        if drop != "plo":
            o = (o + pv(pl, vh[:, :, j])).astype(f32)
        o = ((o + pv(ph, vl[:, :, j])).astype(f32) + pv(ph, vh[:, :, j])).astype(f32)
    out = (o * (f32(1.0) / l_run)).astype(f32)
    return split_rn(out.transpose(0, 2, 1, 3).reshape(B * L, nh * dh), dt)
