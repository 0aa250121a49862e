"""References and per-element error bounds of the kernels a sampling step launches outside the GEMMs and attention: csrc/elementwise.hip,
csrc/norm.hip, csrc/rounding.hip, csrc/headtail.hip and the two rounding helpers at the end of csrc/gemm.hip.  For
tests/test_step_matrix_gpu.py (the kernels against them) and tests/test_step_bound_cpu.py (a float32 / bf16 restatement of every bounded
kernel stays within half of its bound).  Imported by test modules; not a conftest.  numpy only (torch-CPU for the schedule's coefficients).

Three kinds of reference:

A. EXACT.  The diffusion arithmetic (q_sample, the p / ddim update, the slot fold) in numpy float32, one statement at a time in the
   kernels' documented association - those files compile with FP contraction off, every product and sum rounds on its own, and float32
   division is correctly rounded - and plain indexing for the layout movers.  Compared bit for bit.

B. BOUNDED.  float64 of the same formula on the stored inputs, and a bound per element by first-order forward analysis of where the
   kernel rounds, u = 2^-24:
   * output rounding RTOL[dtype] |ref| (2^-8 bf16, 2^-22 fp32), as in tests/train_ref.py;
   * a float32 sum whose longest chain of additions has `depth` links: depth u sum |terms| (`chain_err`).  depth is read off the kernel:
     a lane's own sequential terms plus the levels of the shuffle tree (ln_kernel: 8 ceil(H / 512) + 6; the 16-row panel kernel H / 4 + 2;
     the 4-row one H / 16 + 4; the fused head 16 + 2 + H / 64; a plain n-term loop: n).  numpy's pairwise sum has a shorter chain than
     any of them for n > 8;
   * an fmaf chain or an fp32 MFMA accumulation of K products, in any order: K u sum |products|; the bf16 MFMA chains of head and tail,
     whose order over the K32 steps is the kernel's own loop: 32 u (|partial sum| + sum |products of the step|) per step (`mfma_err`);
   * a lone rounding (the sum of two terms, a product) counts 2 u: the worst case of one correctly rounded operation is u itself, and
     tests/test_step_bound_cpu.py asks the float32 restatement to stay within HALF of every bound;
   * an error that enters a later formula is carried through it with that formula's derivative (LayerNorm: mean -> d -> variance ->
     rstd -> y; the head and tail: the first layer's bf16 intermediate -> the second layer -> LayerNorm);
   * a bf16 intermediate (the tanh slabs of head and tail) may round to the other neighbour than the reference's does only where the
     exact value lies within its own arithmetic error of a rounding boundary: `flip_err` gives those elements one bf16 ulp and the
     others nothing;
   * device expf / sinf / cosf: MATH_ULP units in the last place of the result plus the argument's rounding error times the derivative;
     the hardware exp2 / rcp of tanh_fast: TANH_ABS absolute (1 - 2 / (1 + e): two 1-ulp instructions on values of O(1)).
   An argbest has no bound of its own: `argbest_check` applies the margin rule to the float64 scores with the per-row bound of the
   kernel's score error.

C. The truncated normal (`trunc_normal`): Philox4x32-10 and the rejection loop restated exactly, Box-Muller in float64; the device's
   log / sqrt / sin / cos are hardware instructions, so values agree to a tolerance the matrix measures (and caps at 1e-4).

Nothing here was fitted to what a kernel returned."""
import numpy as np

import gemm_census as gc
import train_ref as tr
from train_ref import BF16, F32, MATH_ULP, RTOL, U, bf16_round, q, ratio  # noqa: F401  (re-exported for the test modules)

TANH_ABS = 16 * U
INT_MAX = 0x7FFFFFFF
f32 = np.float32


def rng(seed):
    return np.random.default_rng(seed)


def chain_err(depth, abs_terms_sum):
    return depth * U * abs_terms_sum


def bf16_ulp(x):
    """spacing of bf16 at |x| (float64 array): 2^(floor(log2 |x|) - 7); the smallest normal's for 0"""
    ax = np.maximum(np.abs(x), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)


def flip_err(x, err):
    """error of bf16(x~) against bf16(x) when |x~ - x| <= err: one ulp where x lies within err of a rounding boundary (the midpoint of
    two neighbouring bf16 values), nothing elsewhere"""
    ulp = bf16_ulp(x)
    frac = np.abs(x) / ulp
    dist = np.abs(frac - np.floor(frac) - 0.5) * ulp          # distance to the nearest midpoint
    return np.where(dist <= err, bf16_ulp(np.abs(x) + err), 0.0)   # (the spacing above a power of two, should the error reach across one)


# ------------------------------------------------------------------------------------------------------------------ schedule
_COEF = {}


def coef_table(kind, eta=0.0):
    """[2000, 8] float32: the mh_step_coef rows of the product's own schedule (sqrt betas, 2000 steps), as the loops upload them"""
    key = (kind, eta)
    if key not in _COEF:
        from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
        d = SpacedDiffusion(use_timesteps=space_timesteps(2000, [2000]), betas=get_named_beta_schedule("sqrt", 2000), rescale_timesteps=True,
                            predict_xstart=True)
        _COEF[key] = d._coef_table(kind, eta, "cpu").numpy().astype(np.float32).copy()
    return _COEF[key]


# ------------------------------------------------------------------------------------------------------------------ A. exact arithmetic
def anchored(mask, shape):
    """mask None | [B, L] | [B, L, E] int32 -> bool [B, L, E]: the elements that keep x_start (mask == 0)"""
    if mask is None:
        return np.zeros(shape, dtype=bool)
    m = np.asarray(mask)
    return np.broadcast_to((m if m.ndim == 3 else m[:, :, None]) == 0, shape)


def q_sample(x0, noise, a, s, mask):
    """x0, noise [B, L, E] float32; a, s [B]: out = a[b] x + s[b] noise (two products, one sum), x where anchored"""
    t1 = a[:, None, None].astype(f32) * x0
    t2 = s[:, None, None].astype(f32) * noise
    return np.where(anchored(mask, x0.shape), x0, t1 + t2).astype(f32)


def step_update(x0, xt, nz, coef, clip, ddim, mask=None, x_start=None):
    """csrc/step_update.h on float32 arrays [B, L, E]; coef [B, 8] or [1, 8] float32 (one row per batch item or one for all); nz None:
    zeros.  -> sample, pred (x0 after the clip), mean.  Every statement rounds on its own."""
    x0, xt = x0.astype(f32), xt.astype(f32)
    nz = np.zeros_like(xt) if nz is None else nz.astype(f32)
    c = np.broadcast_to(coef.astype(f32)[:, None, None, :], x0.shape + (8,))
    if clip:
        x0 = np.minimum(np.maximum(x0, f32(-1.0)), f32(1.0))
    with np.errstate(all="ignore"):
        if ddim:
            eps = (c[..., 3] * xt - x0) / c[..., 4]
            mean = x0 * c[..., 5] + c[..., 6] * eps
        else:
            mean = c[..., 0] * x0 + c[..., 1] * xt
        sample = mean + c[..., 2] * nz
    if mask is not None:
        sample = np.where(anchored(mask, x0.shape), x_start.astype(f32), sample)
    return sample.astype(f32), x0, mean.astype(f32)


def fold_slots(pbest, pidx):
    """[rows, nslots] partial (score, index) -> [rows] index: the larger score, on a tie the smaller index, 0 when nothing was chosen
    (argbest_reduce_kernel and the SLOTS form of step_epilogue4_kernel); a NaN score compares false both ways and is never taken"""
    rows, ns = pbest.shape
    best = np.full(rows, -np.inf, dtype=f32)
    bi = np.full(rows, INT_MAX, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for s in range(ns):
            v, k = pbest[:, s], pidx[:, s].astype(np.int64)
            take = (v > best) | ((v == best) & (k < bi))
            best, bi = np.where(take, v, best), np.where(take, k, bi)
    return np.where(bi == INT_MAX, 0, bi).astype(np.int32)


def pack_panel(a, ld_rows, cols_pad):
    """[rows, cols] float32 -> bf16 K32 panels [cols_pad / 32, ld_rows, 32] as float32, zero outside rows x cols"""
    rows, cols = a.shape
    full = np.zeros((ld_rows, cols_pad), dtype=f32)
    full[:rows, :cols] = bf16_round(a)
    return full.reshape(ld_rows, cols_pad // 32, 32).transpose(1, 0, 2).copy()


def from_panel(p, rows, cols=None):
    """[C / 32, ld, 32] -> [rows, C (or cols)]"""
    a = p.transpose(1, 0, 2).reshape(p.shape[1], -1)[:rows]
    return a if cols is None else a[:, :cols]


def to_panel(a, ld, fill=np.nan):
    """[rows, C] -> [C / 32, ld, 32], rows behind the last hold `fill`"""
    rows, C = a.shape
    p = np.full((C // 32, ld, 32), fill, dtype=f32)
    p[:, :rows] = a.reshape(rows, C // 32, 32).transpose(1, 0, 2)
    return p


def split_table(table, V, E, Vp=768):
    """mh_round_split_table: parts hi | hi | lo as [3 E / 32, Vp, 32] float32 (zero rows beyond V)"""
    full = np.zeros((Vp, E), dtype=f32)
    full[:V] = table
    hi = bf16_round(full)
    lo = bf16_round(full - hi)
    pan = lambda a: a.reshape(Vp, E // 32, 32).transpose(1, 0, 2)
    return np.concatenate([pan(hi), pan(hi), pan(lo)], axis=0)


# ------------------------------------------------------------------------------------------------------------------ C. truncated normal
def u01(r):
    """((float)(r >> 8) + 0.5f) * 2^-24 in float32 (the sum rounds to even above 2^23)"""
    return (((r >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)).astype(f32)


def trunc_normal(n, first, bound, seed, stream_id, step, tol=0.0):
    """trunc_normal4 of elements first .. first + n - 1 (first % 4 == 0): Philox4x32-10 keyed by the seed at counter words
    {g, (g >> 32) | ((attempt >> 8) << 24), step, (stream_id << 8) | (attempt & 0xff)}, g = global group = element / 4; word pairs ->
    Box-Muller in float64 (r0 cos, r0 sin, r1 cos, r1 sin of u01(c0), u01(c1) / u01(c2), u01(c3)); candidate k of a call goes to element k of
    the group if that element is still pending and |candidate| <= bound (bound <= 0: always).
    -> (z float64 [n], near bool [n], attempts): near marks an element for which some candidate it examined lies within `tol` of +-bound
    (the device's last bits may decide the other way there); attempts = the largest attempt number used + 1"""
    ng = (n + 3) // 4
    g = np.arange(ng, dtype=np.uint64) + np.uint64(first // 4)
    z = np.zeros((ng, 4))
    near = np.zeros((ng, 4), dtype=bool)
    pending = np.ones((ng, 4), dtype=bool)
    M32 = np.uint64(0xFFFFFFFF)
    attempt = 0
    while attempt < 1024:
        live = np.nonzero(pending.any(1))[0]
        if live.size == 0:
            break
        gl = g[live]
        c = gc.philox7([gl & M32, (gl >> np.uint64(32)) | np.uint64((attempt >> 8) << 24), np.full(gl.shape, step, np.uint64),
                        np.full(gl.shape, ((stream_id << 8) & 0xFFFFFFFF) | (attempt & 0xFF), np.uint64)], seed & 0xFFFFFFFF, seed >> 32, rounds=10)
        r0 = np.sqrt(-2.0 * np.log(u01(c[0]).astype(np.float64)))
        r1 = np.sqrt(-2.0 * np.log(u01(c[2]).astype(np.float64)))
        a0 = 2.0 * np.pi * u01(c[1]).astype(np.float64)
        a1 = 2.0 * np.pi * u01(c[3]).astype(np.float64)
        cand = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
        p = pending[live]
        if bound > 0:
            ok = np.abs(cand) <= bound
            near[live] |= p & (np.abs(np.abs(cand) - bound) <= tol)
        else:
            ok = np.ones_like(p)
        take = p & ok
        zl = z[live]
        zl[take] = cand[take]
        z[live] = zl
        pending[live] = p & ~ok
        attempt += 1
    return z.reshape(-1)[:n], near.reshape(-1)[:n], attempt


# ------------------------------------------------------------------------------------------------------------------ B. bounded references
def row_sqnorm(x):
    """[rows, E] float32 -> (sum of squares in float64, bound): E products (u each) and a sum of at most E links"""
    s = (x.astype(np.float64) ** 2).sum(1)
    return s, (x.shape[1] + 1) * U * s + 1e-300


def timestep_embedding(t, dim, dtype, max_period=10000.0):
    """t [B] float32 -> [B, 2 (dim / 2)] (cos | sin of t exp(-ln(max_period) k / half)), bound.  The frequency's exponent carries three
    float32 roundings (the host's logf, the product with k, the division) and expf's own; the argument t f one more; the bound is that
    argument error (|d sin|, |d cos| <= 1) plus sinf / cosf's own and the output rounding."""
    half = dim // 2
    k = np.arange(half, dtype=np.float64)
    z = -np.log(max_period) * k / half
    f = np.exp(z)
    a = t.astype(np.float64)[:, None] * f[None]
    ref = np.concatenate([np.cos(a), np.sin(a)], axis=1)
    rel_f = U * (3 * np.abs(z) + MATH_ULP + 1)
    da = np.abs(a) * (rel_f[None] + U)
    da = np.concatenate([da, da], axis=1)
    return ref, da + MATH_ULP * U * np.abs(ref) + RTOL[dtype] * np.abs(ref) + 1e-300


def timestep_embedding_emulate(t, dim, max_period=10000.0):
    half = dim // 2
    nlp = f32(-np.log(f32(max_period)))
    fr = np.exp((nlp * np.arange(half, dtype=f32) / f32(half)).astype(f32)).astype(f32)
    a = (t.astype(f32)[:, None] * fr[None]).astype(f32)
    return np.concatenate([np.cos(a), np.sin(a)], axis=1).astype(f32)


def add_pos_time(x, pos, emb_t, rows_of, L):
    """(pos[l] + x) + emb_t[row of b] in float32, the reference's association: [B L, H] float32 (exact restatement: two rounded sums)"""
    n, H = x.shape
    l = np.arange(n) % L
    b = np.arange(n) // L
    return ((pos[l].astype(f32) + x.astype(f32)) + emb_t[rows_of[b]].astype(f32)).astype(f32)


def ln_depth(H, form="rows"):
    return {"rows": 8 * ((H // 8 + 63) // 64) + 6, "panel16": H // 4 + 2, "panel4": H // 16 + 4, "head": 16 + 2 + H // 64}[form]


def layernorm(v, gamma, beta, eps, dtype, depth, ein=None):
    """v [rows, H] (float32 values as the kernel holds them, or float64 with a per-element error `ein` already in them) -> (y, bound) of
    y = (v - mean) rstd gamma + beta with the two-pass statistics of csrc/norm.hip: mean = sum v / H, var = sum (v - mean)^2 / H,
    rstd = 1 / sqrt(var + eps).  Errors are carried from stage to stage."""
    v = v.astype(np.float64)
    g, b = gamma.astype(np.float64), beta.astype(np.float64)
    H = v.shape[1]
    e0 = np.zeros_like(v) if ein is None else ein
    mean = v.mean(1, keepdims=True)
    e_mean = e0.mean(1, keepdims=True) + chain_err(depth, np.abs(v).sum(1, keepdims=True)) / H + U * np.abs(mean)
    d = v - mean
    e_d = e0 + e_mean + U * np.abs(d)
    var = (d * d).mean(1, keepdims=True)
    e_var = ((2 * np.abs(d) * e_d + e_d * e_d).sum(1, keepdims=True) + chain_err(depth + 1, (d * d).sum(1, keepdims=True))) / H + U * var
    rstd = 1.0 / np.sqrt(var + eps)
    rel_rstd = 0.5 * e_var / (var + eps) + 3 * U
    xhat = d * rstd
    e_xhat = e_d * rstd + np.abs(xhat) * rel_rstd + U * np.abs(xhat)
    y = xhat * g + b
    bound = np.abs(g) * e_xhat + 2 * U * (np.abs(xhat * g) + np.abs(y)) + RTOL[dtype] * np.abs(y) + 1e-300
    return y, bound


def lane_tree_sum(a):
    """sum over the last axis of a [rows, H] float32 in ln_kernel's order: lane l owns the 8-element chunks l, l + 64, ... and adds them in
    turn, then six xor-shuffle levels"""
    rows, H = a.shape
    nper = (H // 8 + 63) // 64
    p = np.zeros((rows, nper * 64 * 8), dtype=f32)
    p[:, :H] = a
    p = p.reshape(rows, nper, 64, 8)
    s = np.zeros((rows, 64), dtype=f32)
    for i in range(nper):
        for e in range(8):
            s = (s + p[:, i, :, e]).astype(f32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ o]).astype(f32)
    return s[:, :1]


def layernorm_emulate(v, gamma, beta, eps, order="lanes"):
    """the kernel's statements in float32 (order "lanes": ln_kernel's own summation order; "numpy": numpy's pairwise one, standing in for
    the panel kernels' 4- and 16-lane trees)"""
    v = v.astype(f32)
    H = f32(v.shape[1])
    sm = lane_tree_sum if order == "lanes" else (lambda a: a.sum(1, keepdims=True, dtype=f32))
    mean = (sm(v) / H).astype(f32)
    d = (v - mean).astype(f32)
    var = (sm((d * d).astype(f32)) / H).astype(f32)
    rstd = (f32(1.0) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)
    return (((d * rstd).astype(f32) * gamma.astype(f32)).astype(f32) + beta.astype(f32)).astype(f32)


def ln_inputs(rows, H, dtype, seed, cancel):
    """rows with a per-row offset (|mean| up to 3) and a per-row scale over 30x; `cancel`: mean 100 and standard deviation 0.01 instead (in
    bf16 storage the spacing at 100 is 0.5 and such a row would be constant, which no bound survives: standard deviation 2 there)"""
    g = rng(seed)
    if cancel:
        x = 100.0 + (0.01 if dtype == F32 else 2.0) * g.standard_normal((rows, H))
    else:
        x = g.uniform(-3, 3, (rows, 1)) + 10.0 ** g.uniform(-1.0, 0.5, (rows, 1)) * g.standard_normal((rows, H))
    x = q(x, dtype)
    assert (x.max(1) > x.min(1)).all(), "a constant row"
    gamma = (1.0 + 0.3 * g.standard_normal(H)).astype(f32)
    beta = (0.2 * g.standard_normal(H)).astype(f32)
    return x, gamma, beta


def pos_time_inputs(B, L, H, seed, with_rows):
    g = rng(seed)
    pos = (0.5 * g.standard_normal((L, H))).astype(f32)
    emb_t = (0.5 * g.standard_normal((B + 2, H))).astype(f32)
    rows_of = ((np.arange(B) + 2) % (B + 2)).astype(np.int32) if with_rows else np.arange(B, dtype=np.int32)
    return pos, emb_t, rows_of


# ---- argbest
def argbest_inputs(n, V, E, seed, dups=True):
    """a table of N(0, 1) rows with duplicated rows where the kernel's tie rules differ (two tx lanes of one 64-row tile, the same lane of
    two tiles, the partial last tile), x = a table row + 0.3 noise (the duplicated rows are targeted first), aux for mode 1"""
    g = rng(seed)
    table = g.standard_normal((V, E)).astype(f32)
    pairs = []
    if dups:
        last = (V - 1) // 64 * 64
        for a, b in ((3, 5), (7, 64 + 7), (9, 128 + 9), (last + 1, last + 12), (20, last + 3), (0, 64)):
            if a < b < V and all(a not in p and b not in p for p in pairs):
                table[b] = table[a]
                pairs.append((a, b))
    target = g.integers(0, V, n)
    flat = [v for p in pairs for v in p[::-1]]        # (the later copy first: the row nearest to it must still round to the earlier one)
    target[:min(n, len(flat))] = flat[:n]
    x = (table[target] + 0.3 * g.standard_normal((n, E))).astype(f32)
    bias = (0.1 * g.standard_normal(V)).astype(f32)
    first_of = np.arange(V)
    for a, b in pairs:
        first_of[b] = a
        bias[b] = bias[a]
    return x, table, bias, first_of, pairs


def round_scores(x, table, tnorm, K=None, split=False):
    """float64 scores -(|T_v|^2 + |x_n|^2 - 2 x.T_v) clamped at 0 from above ([n, V]) and the per-row bound of the kernel's score error:
    the dot product (K fmaf / MFMA links, or with `split` the three bf16 products' dropped terms 3 x 2^-18 plus 3 K links), |x_n|^2,
    the table norm as float32, and the two roundings of the expression.  tnorm: the float32 norms the kernel is given (None: exact)"""
    xd, td = x.astype(np.float64), table.astype(np.float64)
    K = K or x.shape[1]
    dot = xd @ td.T
    S = np.abs(xd) @ np.abs(td).T
    xn = (xd * xd).sum(1, keepdims=True)
    tn = (td * td).sum(1)[None] if tnorm is None else tnorm.astype(np.float64)[None]
    e_dot = ((K + 1) * U + (3.1 * 2.0 ** -18 + 2 * K * U if split else 0.0)) * S
    e_tn = (x.shape[1] + 1) * U * tn if tnorm is None else 0.0
    dist = (tn + xn) - 2 * dot
    e = 2 * e_dot + (x.shape[1] + 2) * U * xn + e_tn + 2 * U * (tn + xn) + 2 * U * np.abs(dist)
    return -np.maximum(dist, 0.0), e.max(1) + 1e-300


def logit_scores(x, table, bias):
    xd, td = x.astype(np.float64), table.astype(np.float64)
    s = xd @ td.T + bias.astype(np.float64)[None]
    e = (x.shape[1] + 1) * U * (np.abs(xd) @ np.abs(td).T) + 2 * U * np.abs(s)
    return s, e.max(1) + 1e-300


def argbest_check(scores, bound, got, first_of=None):
    """the margin rule: -> (number of rows in the second class, list of failures).  Class 1 (best - second best > 2 bound): the index must
    be the float64 argbest (the first copy of it where the table holds identical rows: they are one candidate).  Class 2: the chosen row's float64 score within `bound` of the best.  Everywhere: a row of the table that has
    an identical earlier copy is never chosen (`first_of`)."""
    n, V = scores.shape
    got = np.asarray(got).astype(np.int64)
    bad = []
    if ((got < 0) | (got >= V)).any():
        return 0, ["index out of range at rows %s" % np.nonzero((got < 0) | (got >= V))[0][:8].tolist()]
    ranked = scores
    if first_of is not None:                  # (an identical later copy is no second candidate: its score is the first copy's, exactly)
        ranked = np.where((first_of != np.arange(V))[None], -np.inf, scores)
    order = np.argsort(-ranked, axis=1, kind="stable")
    best = ranked[np.arange(n), order[:, 0]]
    second = ranked[np.arange(n), order[:, 1]] if V > 1 else np.full(n, -np.inf)
    clear = (best - second) > 2 * bound
    chosen = scores[np.arange(n), got]
    w1 = clear & (got != order[:, 0])
    w2 = ~clear & (best - chosen > bound)
    if w1.any():
        r = int(np.nonzero(w1)[0][0])
        bad.append("%d clear rows differ, first row %d: got %d want %d (gap %.3g, bound %.3g)" % (int(w1.sum()), r, got[r], order[r, 0],
                                                                                                  best[r] - second[r], bound[r]))
    if w2.any():
        r = int(np.nonzero(w2)[0][0])
        bad.append("%d near-tie rows chose a row outside the bound, first row %d: got %d (%.9g) best %d (%.9g)" % (
            int(w2.sum()), r, got[r], chosen[r], order[r, 0], best[r]))
    if first_of is not None:
        w3 = first_of[got] != got
        if w3.any():
            r = int(np.nonzero(w3)[0][0])
            bad.append("%d rows chose the later of two identical table rows, first row %d: got %d, its first copy is %d" % (
                int(w3.sum()), r, got[r], first_of[got[r]]))
    return int((~clear).sum()), bad


def vocab_argmax_emulate(x, table, aux, mode):
    """float32 restatement of vocab_argmax_kernel's scores (numpy's float32 matmul for the fmaf chain), first-index argmax"""
    dot = (x.astype(f32) @ table.astype(f32).T).astype(f32)
    if mode == 1:
        s = (dot + aux.astype(f32)[None]).astype(f32)
    else:
        xn = (x.astype(f32) ** 2).sum(1, keepdims=True, dtype=f32)
        s = -np.maximum(((aux.astype(f32)[None] + xn).astype(f32) - f32(2.0) * dot).astype(f32), f32(0.0))
    return s.argmax(1), s


# ---- head and tail of the denoiser
def dense_inputs(n_out, n_in, seed, pad_to=None):
    """bf16-rounded weight [n_out, n_in] (columns beyond n_in up to pad_to: zero) and a float32 bias"""
    g = rng(seed)
    w = np.zeros((n_out, pad_to or n_in), dtype=f32)
    w[:, :n_in] = bf16_round(g.standard_normal((n_out, n_in)) / np.sqrt(n_in))
    return w, (0.1 * g.standard_normal(n_out)).astype(f32)


def mfma_err(a, w):
    """error of the float32 accumulator after the K / 32 chained MFMA steps of a [n, K] . [m, K]^T product of bf16 values (exact products).
    The chain over the K32 steps is the kernels' own (kt = 0, 1, ...): after step kt the accumulator holds P_kt, the sum of the first
    32 (kt + 1) products.  Inside a step the 32 products join the accumulator in an order and grouping the hardware does not document; in
    ANY order, with at least float32 precision per addition, every intermediate is at most |P_kt-1| + sum |products of the step| in
    magnitude and there are at most 32 additions: 32 u (|P_kt-1| + S_kt) per step, summed over the steps"""
    ad, wd = a.astype(np.float64), w.astype(np.float64)
    n, K = ad.shape
    P = np.zeros((n, wd.shape[0]))
    err = np.zeros_like(P)
    for k0 in range(0, K, 32):
        err += np.abs(P) + np.abs(ad[:, k0:k0 + 32]) @ np.abs(wd[:, k0:k0 + 32]).T
        P += ad[:, k0:k0 + 32] @ wd[:, k0:k0 + 32].T
    return 32 * U * err


def tanh_layer(x, w0, b0, flips=True):
    """bf16(tanh(x W0^T + b0)) in float64 and its error: the MFMA chain, the bias sum, tanh_fast's instructions -> `flip_err`
    (flips = False: no error at all - for a restatement that is handed this very intermediate)"""
    xd, wd = x.astype(np.float64), w0.astype(np.float64)
    pre = xd @ wd.T + b0.astype(np.float64)[None]
    e_pre = mfma_err(x, w0) + 2 * U * np.abs(pre)
    h = np.tanh(pre)
    e_h = e_pre * (1 - h * h) + TANH_ABS
    hb = bf16_round(h.astype(f32)).astype(np.float64)
    return hb, flip_err(h, e_h) if flips else np.zeros_like(hb)


def second_layer(h, e_h, w2, b2):
    """h W2^T + b2 in float64 with the first layer's error carried through |W2| plus the MFMA chain's and the bias sum's"""
    wd = w2.astype(np.float64)
    y = h @ wd.T + b2.astype(np.float64)[None]
    e = e_h @ np.abs(wd).T + mfma_err(h, w2) + 2 * U * np.abs(y)
    return y, e


def head(x, E_pad, w0, b0, w2, b2, pos, emb_t, rows_of, L, gamma, beta, eps, flips=True):
    """mh_up_proj_ln_fused: x [rows, E] float32 (rounded to bf16 by the kernel) -> LayerNorm((pos + (tanh(x W0^T + b0) W2^T + b2)) + emb)
    as bf16 panel rows: (y, bound) [rows, H]"""
    n, E = x.shape
    xb = np.zeros((n, E_pad), dtype=f32)
    xb[:, :E] = bf16_round(x)
    h, e_h = tanh_layer(xb, w0, b0, flips)
    y2, e2 = second_layer(h, e_h, w2, b2)
    H = w2.shape[0]
    l, b = np.arange(n) % L, np.arange(n) // L
    v = (pos[l].astype(np.float64) + y2) + emb_t[rows_of[b]].astype(np.float64)
    e_v = e2 + 2 * U * (np.abs(pos[l] + y2) + np.abs(v))
    return layernorm(v, gamma, beta, eps, BF16, ln_depth(H, "head"), ein=e_v)


def tail(X, w0, b0, w2, b2, flips=True):
    """mh_down_proj_fused: X [rows, H] bf16 values -> tanh(X W0^T + b0) W2^T + b2, float32 rows: (y, bound)"""
    h, e_h = tanh_layer(X, w0, b0, flips)
    y, e = second_layer(h, e_h, w2, b2)
    return y, e + RTOL[F32] * np.abs(y) + 1e-300


def dense_emulate(x, w0, b0, w2, b2, own_h=True):
    """the two dense layers in float32 numpy with the bf16 intermediate.  own_h: the intermediate of its own float32 tanh layer (held to
    the whole bound by tests/test_step_bound_cpu.py: a flipped bf16 rounding uses all of its allowance or none); else the reference's
    intermediate (held to half of the bound without the flips)"""
    if own_h:
        h = bf16_round(np.tanh(((x.astype(f32) @ w0.astype(f32).T).astype(f32) + b0.astype(f32)).astype(f32)).astype(f32))
    else:
        h = tanh_layer(x, w0, b0, False)[0].astype(f32)
    return ((h @ w2.astype(f32).T).astype(f32) + b2.astype(f32)).astype(f32)
