"""float64 references, per-element error bounds and float32 restatements of the optimizer kernels of csrc/train.hip (adamw_ema_kernel,
sumsq_chunks_kernel, sum_partials_kernel, clip_grads_kernel), for tests/test_optim_matrix_gpu.py (the kernels through mh_adamw_ema_step /
mh_grad_norm / mh_clip_grads against them) and tests/test_optim_bound_cpu.py (the restatements stay inside the bounds, wrong variants do
not).  Imported by test modules; not a conftest.  numpy only, conventions of tests/train_ref.py: references take the stored float32 inputs
and the float32 fields of mh_opt_hparams AS STORED (the kernel multiplies by those), compute in float64 and come as (ref, bound) pairs.

u = 2^-24 (one fp32 rounding, relative), T = 2^-149 (one rounding in the subnormal range, absolute).

AdamW + EMA element step, the kernel's formula (hp: d = decay_mul, w1 / w2 = one_minus_beta1 / 2, s = step_size, b = bias2_sqrt):

    pd = p d      m1 = m b1 + g w1      v1 = v b2 + g^2 w2      den = sqrt(v1) / b + eps      p1 = pd - s m1 / den      e1 = e r + p1 (1 - r)

Bounds, from where the kernel rounds (two products and a sum for m1; g g, its product with w2, v b2 and the sum for v1; ...):

    dm   = u (|m b1| + |g w1| + |m1|) + 3 T
    dv   = u (|v b2| + 2 g^2 w2 + |v1|) + 3 T
    dq   = min(dv / (2 sqrt v1), sqrt dv) / b + 2 u q + T,  q = sqrt(v1) / b     (sqrt is 1/2-Lipschitz in relative terms, and
                                                                                 |sqrt(a) - sqrt(a')| <= sqrt |a - a'| near zero)
    dden = dq + u den
    dr   = dm / den + |r| dden / den + u |r| + T,  r = m1 / den
    dp   = u |pd| + s dr + u s |r| + u |p1| + 3 T
    de   = u (|e r| + |p1 (1 - r)| + |e1|) + 3 T + (1 - r) dp                    (a NULL-gradient tensor's p is exact: dp = 0)

dm, dv, dp and de are multiplied by SECOND = 1.25 for the second-order terms the first-order analysis drops.  Terms beyond the issue's
derivation: the 3 T of de (its two products and the sum can land in the subnormal range exactly like m1's; without it an EMA copy of
1e-40-sized values would be held to an error float32 cannot meet) - nothing else.

Sum of squares: every term is non-negative, so an fp32 sum in ANY order has relative error at most gamma(D) = D u / (1 - D u), D = the
longest chain of roundings one term passes through (`chunk_depth`, `total_depth`: the product, the 4-term tree (2), one accumulation per
1024-element sweep, the tail add, 6 wave levels, 2 block adds; in sum_partials_kernel ceil(n_chunks / 256) + 6 + 2).  A product that
underflows costs up to T absolutely: `count T` per chunk (named term: the g^2 of |g| < 1e-19 are subnormal).  The norm's relative bound
is gamma (1 + gamma) / 2 + u: sqrt halves a relative error to first order (1 - sqrt(1 - x) <= x (1 + x) / 2 for x < 1/2 covers the
rest), and sqrtf is correctly rounded.

The restatements (`*_restate`) do the kernel's operations in float32 numpy in the kernel's order.  The kernels are compiled under
`#pragma clang fp contract(off)`, HIP's fp32 divide and square root are correctly rounded by default: where a kernel only multiplies and
adds (m, v, the EMA copies, the squares' sums, the clip) the restatement predicts its bits.

Nothing here was fitted to what a kernel returned."""
import math

import numpy as np

U = 2.0 ** -24
T = 2.0 ** -149
SECOND = 1.25
F = np.float32
CLIP_EPS = F(1e-6)
RATES = (0.5, 0.9, 0.99, 0.9999)
GUARD = 64          # NaN elements in front of and behind every tensor of an arena (a multiple of 4: 16-byte alignment is kept)

SIZES = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 1027, 65535, 65536, 65537, 2 * 65536 + 3)
NULLS = {
    "none": (),
    "first": (0,),
    "last": (len(SIZES) - 1,),                                   # 2 * 65536 + 3 elements: several chunks in every table but "one"
    "between": (9,),
    "allbut": tuple(i for i in range(len(SIZES)) if i != 12),    # one live tensor, 1027 elements
    "span": (15,),                                               # 65537 elements between two live tensors
}
N_SPECIAL = (1, 63, 64, 65, 255, 256, 257, 1000)


def ignore():
    return np.errstate(all="ignore")


# ------------------------------------------------------------------------------------------------------------------ hyper-parameters
def hparams(lr, wd, step, n_ema=0, betas=(0.9, 0.999), eps=1e-8):
    """mh_opt_hparams as include/musehip.h defines it: every derived scalar in double, stored as float32"""
    b1, b2 = betas
    return {"beta1": F(b1), "beta2": F(b2), "eps": F(eps), "one_minus_beta1": F(1.0 - b1), "one_minus_beta2": F(1.0 - b2),
            "decay_mul": F(1.0 - lr * wd), "step_size": F(lr / (1.0 - b1 ** step)), "bias2_sqrt": F(math.sqrt(1.0 - b2 ** step)),
            "n_ema": int(n_ema), "ema_rate": [F(r) for r in RATES[:n_ema]], "ema_one_minus": [F(1.0 - r) for r in RATES[:n_ema]]}


# ------------------------------------------------------------------------------------------------------------------ tables
class Layout:
    """tensor sizes, which of them have no gradient, a chunk table (tensor, count, offset) and where each tensor lies in an arena.
    `flat` coordinates: all tensors one after the other; `aidx[flat index]` = arena index."""

    def __init__(self, name, sizes, nulls, chunks):
        self.name, self.sizes, self.nulls = name, tuple(sizes), tuple(sorted(nulls))
        self.chunks = np.asarray(chunks, dtype=np.int64).reshape(-1, 3)
        self.start = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n = int(self.start[-1])
        offs, pos = [], GUARD
        for s in self.sizes:
            offs.append(pos)
            pos += (s + 3) // 4 * 4 + GUARD
        self.offs, self.arena = np.asarray(offs, dtype=np.int64), pos
        self.aidx = np.concatenate([o + np.arange(s) for o, s in zip(self.offs, self.sizes)])
        self.live = np.ones(self.n, dtype=bool)
        for i in self.nulls:
            self.live[self.sl(i)] = False
        t, c, o = self.chunks.T
        self.cstart = self.start[t] + o                        # flat start of every chunk
        self.clive = ~np.isin(t, self.nulls)
        cover = np.zeros(self.n, dtype=np.int64)               # (the table must be a partition, with offsets the kernels may assume)
        np.add.at(cover, np.concatenate([s + np.arange(k) for s, k in zip(self.cstart, c)]), 1)
        assert (cover == 1).all() and (o % 4 == 0).all() and (c > 0).all() and (o + c <= np.asarray(self.sizes)[t]).all()

    def sl(self, i):
        return slice(int(self.start[i]), int(self.start[i + 1]))

    def tail_mask(self):
        """flat elements that a chunk handles in its count % 4 tail loop"""
        m = np.zeros(self.n, dtype=bool)
        for s, k in zip(self.cstart, self.chunks[:, 1]):
            m[s + (k & ~3):s + k] = True
        return m

    def chunk_mask(self, k):
        m = np.zeros(self.n, dtype=bool)
        m[self.cstart[k]:self.cstart[k] + self.chunks[k, 1]] = True
        return m


def split(sizes, piece):
    return [(i, min(piece, n - off), off) for i, n in enumerate(sizes) for off in range(0, n, piece)]


def layout(table, nulls="none"):
    """table: "one" (a chunk per tensor), "host" (65536-element chunks in tensor order, as FusedAdamWEMA builds them), "c8" / "c1028"
    (8- and 1028-element chunks), "shuffled" (the 1028-element table in a fixed random order: tensors interleaved), or "n<k>": k chunks of
    8 elements over two tensors, the last chunk 5 elements long (sum_partials_kernel's stride loop at k > 256)"""
    if table.startswith("n"):
        k = int(table[1:])
        sizes = (8,) if k == 1 else (8 * (k // 2), 8 * (k - k // 2) - 3)
        null = {"none": (), "first": (0,), "last": (len(sizes) - 1,)}[nulls]
        lay = Layout(table, sizes, null, split(sizes, 8))
        assert len(lay.chunks) == k
        return lay
    piece = {"one": 1 << 30, "host": 65536, "c8": 8, "c1028": 1028, "shuffled": 1028}[table]
    chunks = split(SIZES, piece)
    if table == "shuffled":
        chunks = [chunks[i] for i in np.random.default_rng(1028).permutation(len(chunks))]
    return Layout(table, SIZES, NULLS[nulls], chunks)


# ------------------------------------------------------------------------------------------------------------------ inputs
GSCALE = {"s1": 1.0, "s1e-4": 1e-4, "s1e-8": 1e-8, "s1e-12": 1e-12, "s1e6": 1e6, "nonfinite": 1.0}
NAN_AT = (12, 2)         # tensor 12 (1027 elements), element 2: inside a 16-byte piece
INF_AT = (12, 1026)      # ... and its last element: the count % 4 tail of every table


def adam_inputs(lay, step, gkind, seed, scale=None):
    """flat float32 p, g, m, v and e [4, n].  Moments are zero at step 1, else of the gradient's scale.  Special elements, everywhere:
    g = 0 (every 13th; every 26th with zero moments too: den = eps), m b1 = -g w1 (every 17th), a subnormal g^2 (every 19th: |g| = 1e-22,
    the next 3e-23).  gkind "nonfinite": one NaN and one inf gradient element.  A NULL-gradient tensor's moments are NaN in its first half (a
    computed value written there shows) and finite behind it (a decayed moment shows)"""
    r = np.random.default_rng(seed)
    n, sc = lay.n, GSCALE[gkind] if scale is None else scale
    p = r.standard_normal(n).astype(F)
    g = (sc * r.standard_normal(n)).astype(F)
    if step == 1:
        m, v = np.zeros(n, F), np.zeros(n, F)
    else:
        m = (0.3 * sc * r.standard_normal(n)).astype(F)
        v = (sc * sc * r.uniform(0.01, 1.0, n)).astype(F)
    e = (p[None] + 0.1 * r.standard_normal((4, n))).astype(F)
    i = np.arange(n)
    hp = hparams(1e-3, 0.0, step)
    with ignore():
        g[i % 17 == 1] = (-(m * hp["beta1"]) / hp["one_minus_beta1"])[i % 17 == 1]
    g[i % 19 == 2] = F(1e-22)
    g[i % 19 == 3] = F(-3e-23)
    g[i % 13 == 0] = 0
    m[i % 26 == 0] = 0
    v[i % 26 == 0] = 0
    if gkind == "nonfinite":
        g[lay.start[NAN_AT[0]] + NAN_AT[1]] = np.nan
        g[lay.start[INF_AT[0]] + INF_AT[1]] = np.inf
    for t in lay.nulls:
        s = lay.sl(t)
        half = s.start + (lay.sizes[t] + 1) // 2
        m[s.start:half] = np.nan
        v[s.start:half] = np.nan
        m[half:s.stop] = F(0.25)
        v[half:s.stop] = F(0.0625)
        g[s] = np.nan                                          # (no buffer behind it: nothing may depend on this)
    return p, g, m, v, e


def norm_inputs(lay, gkind, seed):
    """flat gradients.  "s1": N(0, 1).  "small": 1e-7 N(0, 1) (a norm of the order of the clip's 1e-6).  "tail": the count % 4 tail elements
    of the table's chunks carry almost all of the norm (1e3 against 1e-3).  "chunk": one 8-element chunk (the middle live one) does.
    "nan" / "inf": one such element"""
    r = np.random.default_rng(seed)
    g = r.standard_normal(lay.n).astype(F)
    if gkind == "small":
        g *= F(1e-7)
    elif gkind == "tail":
        t = lay.tail_mask()
        g = np.where(t, g * F(1e3), g * F(1e-3)).astype(F)
    elif gkind == "chunk":
        g = np.where(lay.chunk_mask(heavy_chunk(lay)), g * F(1e3), g * F(1e-3)).astype(F)
    elif gkind in ("nan", "inf"):
        live = np.nonzero(lay.live)[0]
        g[live[len(live) // 2]] = np.nan if gkind == "nan" else np.inf
    return g


def heavy_chunk(lay):
    live = np.nonzero(lay.clive)[0]
    return int(live[len(live) // 2])


# ------------------------------------------------------------------------------------------------------------------ AdamW + EMA
def adamw_restate(p, g, m, v, hp):
    """adamw_elem of csrc/train.hip in float32, operation for operation -> p1, m1, v1"""
    with ignore():
        pd = p * hp["decay_mul"]
        m1 = m * hp["beta1"] + g * hp["one_minus_beta1"]
        v1 = v * hp["beta2"] + (g * g) * hp["one_minus_beta2"]
        den = np.sqrt(v1) / hp["bias2_sqrt"] + hp["eps"]
        p1 = pd - hp["step_size"] * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == F
    return p1, m1, v1


def ema_restate(e, p1, rate, one_minus):
    with ignore():
        out = e * rate + p1 * one_minus
    assert out.dtype == F
    return out


def adamw_ref(p, g, m, v, hp):
    """-> {"p": (ref, bound), "m": ..., "v": ..., "dp": the bound of p (for the EMA copies)}; elements with a non-finite g give NaN"""
    b1, b2, eps, w1, w2, d, s, b = (float(hp[k]) for k in ("beta1", "beta2", "eps", "one_minus_beta1", "one_minus_beta2", "decay_mul",
                                                           "step_size", "bias2_sqrt"))
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    with ignore():
        pd = p * d
        m1 = m * b1 + g * w1
        v1 = v * b2 + g * g * w2
        root = np.sqrt(v1)
        q = root / b
        den = q + eps
        r = m1 / den
        p1 = pd - s * r
        dm = U * (np.abs(m * b1) + np.abs(g * w1) + np.abs(m1)) + 3 * T
        dv = U * (np.abs(v * b2) + 2 * g * g * w2 + np.abs(v1)) + 3 * T
        dq = np.minimum(np.where(v1 > 0, dv / (2 * root), np.inf), np.sqrt(dv)) / b + 2 * U * q + T
        dden = dq + U * den
        dr = dm / den + np.abs(r) * dden / den + U * np.abs(r) + T
        dp = U * np.abs(pd) + s * dr + U * s * np.abs(r) + U * np.abs(p1) + 3 * T
    return {"p": (p1, SECOND * dp), "m": (m1, SECOND * dm), "v": (v1, SECOND * dv)}


def ema_ref(e, p1, dp, rate, one_minus):
    """e r + p1 (1 - r) with r and 1 - r the stored floats; p1 the float64 reference of the parameter and dp its (final) bound"""
    e, r, om = e.astype(np.float64), float(rate), float(one_minus)
    with ignore():
        e1 = e * r + p1 * om
        de = SECOND * (U * (np.abs(e * r) + np.abs(p1 * om) + np.abs(e1)) + 3 * T) + om * dp
    return e1, de


def ratio(got, ref, bound, mask=None):
    """worst |got - ref| / bound over the elements of mask (an exact zero error counts as 0)"""
    with ignore():
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        r = np.where(err == 0, 0.0, err / bound)
    if mask is not None:
        r = r[mask]
    assert not np.isnan(r).any(), "a NaN among the judged elements"
    return float(r.max()) if r.size else 0.0


def same_bits(a, b):
    """float32 arrays: equal bit for bit, a NaN on both sides counting as equal (payloads are not part of any contract)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _outside(what, got, pair, mask, fails):
    ref, bound = pair
    r = ratio(got, ref, bound, mask)
    if r > 1.0:
        with ignore():
            err = np.where(mask, np.abs(np.asarray(got, dtype=np.float64) - ref) / bound, 0.0)
        i = int(np.argmax(err))
        fails.append("%s: %d elements outside their bound, worst %.3f at flat index %d: got %.9g ref %.9g bound %.3g"
                     % (what, int((err > 1).sum()), r, i, got[i], ref[i], bound[i]))
    return r


def _differs(what, got, want, mask, fails):
    bad = ~same_bits(got, want) & mask
    if bad.any():
        i = int(np.argmax(bad))
        fails.append("%s: %d of %d elements differ in bits, first at flat index %d: got %r want %r" % (what, int(bad.sum()), int(mask.sum()), i,
                                                                                                     got[i], want[i]))


def judge_adam(lay, inputs, hp, got_p, got_m, got_v, got_e):
    """everything tests/test_optim_matrix_gpu.py asserts of one mh_adamw_ema_step call's outputs (flat coordinates; got_e: the n_ema copies)
    -> (worst err / bound per output, share of live p elements bit-equal to the restatement, failed checks)"""
    p, g, m, v, e = inputs
    fails, worst = [], {}
    live = lay.live
    fin = live & np.isfinite(g)
    _differs("p of NULL-gradient tensors", got_p, p, ~live, fails)
    _differs("m of NULL-gradient tensors", got_m, m, ~live, fails)
    _differs("v of NULL-gradient tensors", got_v, v, ~live, fails)
    rp, rm, rv = adamw_restate(p, g, m, v, hp)
    _differs("m against the restatement", got_m, rm, live, fails)
    _differs("v against the restatement", got_v, rv, live, fails)
    ref = adamw_ref(p, g, m, v, hp)
    for k, got in (("p", got_p), ("m", got_m), ("v", got_v)):
        worst[k] = _outside(k, got, ref[k], fin, fails)
    # a non-finite gradient element: its own outputs are what IEEE arithmetic makes of it (m, v: the restatement's bits; p: NaN) - no other
    if not np.isnan(got_p[live & ~fin]).all() or np.isnan(got_p[fin]).any():
        fails.append("p: NaN elements are not exactly those with a non-finite gradient")
    p_ref = np.where(live, ref["p"][0], p.astype(np.float64))
    dp = np.where(live, ref["p"][1], 0.0)
    everywhere = np.ones(lay.n, dtype=bool)
    for k in range(hp["n_ema"]):
        r, om = hp["ema_rate"][k], hp["ema_one_minus"][k]
        _differs("ema %d against fl(fl(e r) + fl(p' (1 - r)))" % k, got_e[k], ema_restate(e[k], got_p, r, om), everywhere, fails)
        worst["e%d" % k] = _outside("ema %d" % k, got_e[k], ema_ref(e[k], p_ref, dp, r, om), fin | ~live, fails)
    return worst, float(same_bits(got_p, rp)[live].mean()), fails


def judge_norm(lay, g, got_part, got_norm):
    """-> (worst err / bound of the partials, of the norm, failed checks)"""
    fails = []
    (pref, pb), (nref, nb) = sumsq_ref(lay, g)
    if not (np.ascontiguousarray(got_part[~lay.clive], dtype=F).view(np.uint32) == 0).all():
        fails.append("the partial of a NULL-gradient chunk is not 0.0f")
    finite = np.isfinite(pref)
    wp = _outside("partial", got_part, (pref, pb), finite, fails)
    if not same_bits(np.asarray(got_part, dtype=F)[~finite], pref[~finite].astype(F)).all():
        fails.append("partial: the chunk with a NaN / inf element does not hold %r" % pref[~finite].tolist())
    if math.isfinite(nref):
        wn = abs(float(got_norm) - nref) / nb if nb > 0 else float(got_norm != nref)
        if not wn <= 1.0:
            fails.append("norm %.9g against %.9g: %.3f of its bound %.3g" % (got_norm, nref, wn, nb))
    else:
        wn = 0.0
        if not same_bits(np.array([got_norm], F), np.array([nref], F)).all():
            fails.append("norm %r, expected %r" % (got_norm, nref))
    return wp, wn, fails


def judge_clip(lay, g, norm, max_norm, got):
    """-> (coef, failed checks): every gradient element bit-equal to the prediction made from the norm the kernel wrote"""
    fails = []
    want, coef = clip_restate(lay, g, norm, max_norm)
    _differs("gradient against fl(g coef), coef %r" % coef, got, want, np.ones(lay.n, dtype=bool), fails)
    return coef, fails


# ------------------------------------------------------------------------------------------------------------------ sum of squares
def gamma(D):
    return D * U / (1.0 - D * U)


def chunk_depth(count):
    n4 = int(count) >> 2
    return 1 + (2 + (n4 + 255) // 256 if n4 else 0) + (1 if count & 3 else 0) + 6 + 2


def total_depth(lay):
    live = lay.chunks[lay.clive, 1]
    return (max(chunk_depth(c) for c in live) if live.size else 0) + (len(lay.chunks) + 255) // 256 + 6 + 2


def sumsq_ref(lay, g):
    """-> (partial ref [n_chunks], bound), (norm ref, bound); a NULL-gradient chunk's partial is exactly 0 (bound 0)"""
    g2 = np.where(lay.live, g.astype(np.float64), 0.0) ** 2
    part = np.empty(len(lay.chunks))
    with ignore():
        for k, (s, c) in enumerate(zip(lay.cstart, lay.chunks[:, 1])):
            part[k] = g2[s:s + c].sum() if lay.clive[k] else 0.0
        pb = np.array([gamma(chunk_depth(c)) * S + c * T if l else 0.0 for c, S, l in zip(lay.chunks[:, 1], part, lay.clive)])
    S = float(part.sum())
    norm = math.sqrt(S) if S == S else float("nan")
    gm = gamma(total_depth(lay))
    nb = norm * (gm * (1 + gm) / 2 + U) + (int(lay.live.sum()) * T / (2 * norm) if 0 < norm < float("inf") else 0.0)
    return (part, pb), (norm, nb)


def _block_reduce(lanes):
    """[N, 256] per-thread float32 values -> [N]: wave_sum's xor butterfly over 64 lanes, then (red0 + red1) + (red2 + red3)"""
    v = lanes.reshape(-1, 4, 64)
    idx = np.arange(64)
    with ignore():
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, idx ^ o]
        red = v[:, :, 0]
        return (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])


def sumsq_restate(lay, g, drop_tail=False):
    """sumsq_chunks_kernel in float32, in the kernel's order, chunks of equal count batched -> partial [n_chunks] float32"""
    out = np.zeros(len(lay.chunks), F)
    counts = lay.chunks[:, 1]
    with ignore():
        for c in np.unique(counts[lay.clive]):
            ks = np.nonzero(lay.clive & (counts == c))[0]
            G = g[lay.cstart[ks][:, None] + np.arange(c)[None]]
            n4 = int(c) >> 2
            lanes = np.zeros((len(ks), 256), F)
            if n4:
                sq = G[:, :n4 * 4].reshape(len(ks), n4, 4)
                sq = sq * sq
                tree = (sq[:, :, 0] + sq[:, :, 1]) + (sq[:, :, 2] + sq[:, :, 3])
                rows = (n4 + 255) // 256
                pad = np.zeros((len(ks), rows * 256), F)
                pad[:, :n4] = tree
                pad = pad.reshape(len(ks), rows, 256)
                lanes = pad[:, 0].copy()                       # (0 + x is exact: the kernel's s = 0.f start adds nothing)
                for r in range(1, rows):
                    lanes = lanes + pad[:, r]                  # (a lane whose sweep is over adds nothing: + 0 is exact)
            if c & 3 and not drop_tail:
                t = G[:, n4 * 4:]
                lanes[:, :t.shape[1]] = lanes[:, :t.shape[1]] + t * t
            out[ks] = _block_reduce(lanes)
    assert out.dtype == F
    return out


def norm_restate(partial, skip=None):
    """sum_partials_kernel in float32: thread t adds partial[t], partial[t + 256], ... in order; the block fold; sqrtf"""
    part = np.asarray(partial, dtype=F)
    if skip is not None:
        part = np.delete(part, skip)
    rows = (part.size + 255) // 256
    pad = np.zeros(rows * 256, F)
    pad[:part.size] = part
    pad = pad.reshape(rows, 256)
    lanes = pad[0].copy()
    with ignore():
        for r in range(1, rows):
            lanes = lanes + pad[r]
        return np.sqrt(_block_reduce(lanes[None]))[0]


# ------------------------------------------------------------------------------------------------------------------ clip
def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6f)) in float32 as torch.nn.utils.clip_grad_norm_ forms it: clamp(max = 1) keeps a NaN"""
    with ignore():
        return np.minimum(F(1.0), F(max_norm) / (F(norm) + CLIP_EPS))


def clip_restate(lay, g, norm, max_norm):
    """the gradients after mh_clip_grads: fl32(g coef) where a gradient exists; the original bits when coef >= 1"""
    coef = clip_coef(norm, max_norm)
    if coef >= 1.0:
        return g.copy(), coef
    with ignore():
        return np.where(lay.live, g * coef, g).astype(F), coef
