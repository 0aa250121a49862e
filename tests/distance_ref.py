"""float64 references and per-element error bounds of the distance-logit kernels (csrc/distance_logits.hip, vocab_argmax_kernel<2> of
csrc/rounding.hip), for tests/test_distance_matrix_gpu.py (the kernels against them) and tests/test_distance_bound_cpu.py (a float32
restatement of each kernel's arithmetic stays within half of them).  Imported by test modules; not a conftest.  numpy only.  The style,
U, RTOL, MATH_ULP, `sum_err` and `_exp_err` are tests/train_ref.py's.

The score of position n against table row v is s = -sqrt(max(d2, 0)) with d2 = (wn[v] + xn[n]) - 2 dot[n][v] evaluated in fp32.

* d2.  wn, xn and dot are fp32 sums of E products each (any order: the exact-fp32 MFMA's, a wave tree's, an fmaf chain's), then one add, one
  subtract; the square root behind it is one more rounding (relative u in s = 2 u in d2).  First order:
      |d2_fp32 - d2| <= delta = (E + 3) EPS32 (wn + xn + 2 sum_i |w_i x_i|),   EPS32 = 2^-23.
  The float64 d2 itself is evaluated as sum_i (x_i - w_i)^2: the same number without the cancellation, and exactly 0 for a position that
  IS a table row.
* s.  delta is carried through the square root with its derivative, delta / (2 sqrt(d2)); where d2 <= delta the derivative is no guide
  and the bound is sqrt(delta) (the computed d2 lies in [0, d2 + delta], clamped or not).
* log-sum-exp.  d lse / d s_v = p_v: sum_v p_v e_s[v], plus expf / logf and the fp32 sum as in train_ref.ce_fwd.
* clamp-uncertain elements: d2 <= delta - whether the kernel's own d2 comes out above 0 cannot be told.  The forward bounds cover them
  (sqrt(delta)); the backward, whose G = dl / (2 s) is 0 on one side and of order 1 / sqrt(delta) on the other, is compared on every OTHER
  element, and a row / column sum that contains such an element is compared with the kernel's own value of it put into the reference sum.
  Where the kernel's fp32 d2 is <= 0 (the test evaluates the same fp32 expression on the same product: bit for bit) G must be exactly 0.
* argmax: the float64 first index of the maximum; a row is low-margin when its float64 top-two gap is at most twice the largest score bound
  of the row, and only the other rows are compared.

Nothing here was fitted to what a kernel returned."""
import numpy as np

from train_ref import FLT_MIN, MATH_ULP, RTOL, F32, U, _exp_err, sum_err, ratio, rng  # noqa: F401

EPS32 = 2.0 ** -23
EMB_STD = 0.5          # the table's scale (oracle.fixtures.EMB_STD)
NEAR = 0.01            # how far the decoder-NLL rows lie from their target row (_get_x_start's own jitter, 0.12 at the sqrt schedule, cancels less)
PAD_FILL = 3.0e30      # what the padding columns of `dots` hold in the tests
CAP = 0.01             # at most this share of clamp-uncertain elements / low-margin rows per case

VS = ((729, 768), (97, 128), (64, 64), (65, 128))      # (V, ld)
NS = (1, 63, 64, 65, 200)
ES = (32, 128, 500)


# ------------------------------------------------------------------------------------------------------------------ inputs
# seeds: the first salt (0, 1, ...) at which the float64 reference alone leaves at most CAP of the case's rows low-margin (a random position's
# two nearest of 729 rows can lie closer together than the score bound); tests/test_distance_bound_cpu.py holds every case to the caps
SALT = {(65, 500, 64): 1}


def case_inputs(V, E, N):
    """-> W [V, E], x [N, E], ids [N], g [N] (float32 / int32).  Row kinds in turn: a random position; a table row exactly, id = that
    row (the clamp on the target); a table row exactly, id = another row; W[id] + 0.01 noise (the decoder-NLL regime, where the
    difference cancels).  A single position (N = 1) sits on its target's row where one element in V stays under CAP (V > 100) and next
    to it otherwise.  g: mixed signs, every fifth 0."""
    r = rng(V * 1009 + E * 13 + N + 100003 * SALT.get((V, E, N), 0))
    W = (EMB_STD * r.standard_normal((V, E))).astype(np.float32)
    ids = r.integers(0, V, N).astype(np.int32)
    x = (EMB_STD * r.standard_normal((N, E))).astype(np.float32)
    kind = (np.arange(N) + V + E) % 4 if N > 1 else np.array([1 if V > 100 else 3])
    x[kind == 1] = W[ids[kind == 1]]
    on = (ids + 1 + r.integers(0, V - 1, N)) % V                       # another row than ids
    x[kind == 2] = W[on[kind == 2]]
    near = (W[ids] + np.float32(NEAR) * r.standard_normal((N, E)).astype(np.float32)).astype(np.float32)
    x[kind == 3] = near[kind == 3]
    g = (2 * r.standard_normal(N)).astype(np.float32)
    g[(np.arange(N) + V) % 5 == 0] = 0.0
    return W, x, ids, g


def tie_inputs(V, E, N):
    """a table in which every third row of the first half has a copy at the far end (a later index), and positions next to - every fourth
    exactly on - such a pair: both rows score the same bit for bit.  -> W, x, first [N]: the lower index of each position's pair"""
    r = rng(V * 7 + E + N)
    W = (EMB_STD * r.standard_normal((V, E))).astype(np.float32)
    src = np.arange(0, V // 2, 3)
    dst = V - 1 - np.arange(len(src))                                   # copies live at the far end: another 64-row tile, another lane
    W[dst] = W[src]
    pick = r.integers(0, len(src), N)
    x = (W[dst[pick]] + np.float32(0.05) * r.standard_normal((N, E)).astype(np.float32)).astype(np.float32)
    x[::4] = W[dst[pick[::4]]]                                          # and exactly on the pair
    return W, x, src[pick].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ scores
def scores(x, W):
    """-> s [N, V], e_s (its bound), d2, delta, uncertain (d2 <= delta)"""
    x, W = x.astype(np.float64), W.astype(np.float64)
    E = x.shape[1]
    wn, xn = (W * W).sum(1), (x * x).sum(1)
    A = np.abs(x) @ np.abs(W).T
    d2 = ((x[:, None, :] - W[None, :, :]) ** 2).sum(-1) if x.shape[0] * W.shape[0] * E <= 1 << 24 else _d2_blocked(x, W)
    delta = (E + 3) * EPS32 * (wn[None, :] + xn[:, None] + 2 * A)
    unc = d2 <= delta
    s = -np.sqrt(d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(unc, np.sqrt(delta), delta / (2 * np.sqrt(d2)))
    return s, e_s, d2, delta, unc


def _d2_blocked(x, W):
    out = np.empty((x.shape[0], W.shape[0]))
    for i in range(0, x.shape[0], 16):
        out[i:i + 16] = ((x[i:i + 16, None, :] - W[None, :, :]) ** 2).sum(-1)
    return out


def ce_fwd(x, W, ids):
    """-> {"lse": (ref, bound), "nll": (ref, bound)} and the scores tuple"""
    sc = scores(x, W)
    s, e_s = sc[0], sc[1]
    n, V = s.shape
    mx = s.max(1, keepdims=True)
    z = s - mx
    e = np.exp(z)
    S = e.sum(1, keepdims=True)
    p = e / S
    e_S = _exp_err(e, z).sum(1, keepdims=True) + sum_err(V, S)
    lse = (mx + np.log(S))[:, 0]
    e_lse = (p * e_s).sum(1) + (e_S / S + U + MATH_ULP * U * np.abs(np.log(S)))[:, 0] + U * (np.abs(mx[:, 0]) + np.abs(lse))
    r = np.arange(n)
    nll = lse - s[r, ids]
    e_nll = e_lse + e_s[r, ids] + U * np.abs(nll)
    return {"lse": (lse, e_lse + RTOL[F32] * np.abs(lse)), "nll": (nll, e_nll + RTOL[F32] * np.abs(nll))}, sc


def ce_bwd(x, W, ids, lse, g, sc=None):
    """lse, g: the fp32 values the kernel is given.  -> G (ref, bound) [N, V] with 0 / 0 at the clamp-uncertain elements, and `unc`.
    d_dots = -2 G (exact scaling: twice the bound), d_xn / d_wn through `g_sums`."""
    s, e_s, d2, delta, unc = sc if sc is not None else scores(x, W)
    n, V = s.shape
    z = s - lse.astype(np.float64)[:, None]
    p = np.exp(z)
    e_p = _exp_err(p, z) + p * e_s
    oh = np.zeros_like(p)
    oh[np.arange(n), ids] = 1.0
    gs = g.astype(np.float64)[:, None]
    dl = gs * (p - oh)
    e_dl = np.abs(gs) * (e_p + U * np.abs(p - oh)) + U * np.abs(dl)
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.where(unc, 0.0, dl / (2 * s))
        e_G = np.where(unc, 0.0, e_dl / (2 * np.abs(s)) + np.abs(G) * e_s / np.abs(s) + 2 * U * np.abs(G))
    return (G, e_G + RTOL[F32] * np.abs(G)), unc


def g_sums(G, e_G, unc, G_got, axis):
    """sum of G over `axis` (1: d_xn [N], 0: d_wn [V]) with the kernel's own G at the clamp-uncertain elements -> (ref, bound)"""
    terms = np.where(unc, np.asarray(G_got, dtype=np.float64), G)
    ref = terms.sum(axis)
    n = G.shape[axis] + 1
    return ref, e_G.sum(axis) + sum_err(n, np.abs(terms).sum(axis)) + RTOL[F32] * np.abs(ref)


def sqnorm_bwd(x, c, c_scale):
    """2 (c_scale c[r]) x[r][:]: c_scale is a power of two, so one rounding of the product and none before it"""
    ref = 2.0 * float(c_scale) * c.astype(np.float64)[:, None] * x.astype(np.float64)
    return ref, U * np.abs(ref) + RTOL[F32] * np.abs(ref)


def argmax(x, W, sc=None):
    """-> idx [N] (float64 first index of the maximum), safe [N] (top-two gap > twice the row's largest score bound)"""
    s, e_s = (sc if sc is not None else scores(x, W))[:2]
    idx = s.argmax(1)
    if s.shape[1] == 1:
        return idx, np.ones(len(idx), dtype=bool)
    top2 = np.partition(s, -2, axis=1)[:, -2:]
    return idx, (top2[:, 1] - top2[:, 0]) > 2 * e_s.max(1)


# ------------------------------------------------------------------------------------------------------------------ float32 restatements
def dots_emulate(x, W):
    """the fp32 product and squared norms (summation order numpy's) -> dots, wn, xn"""
    f = np.float32
    x, W = x.astype(f), W.astype(f)
    return x @ W.T, (W * W).sum(1, dtype=f), (x * x).sum(1, dtype=f)


def d2_emulate(dots, wn, xn):
    """the kernels' own expression on the values they are given: bit for bit the device's d2 (no contraction there)"""
    f = np.float32
    return (wn.astype(f)[None, :] + xn.astype(f)[:, None]) - f(2.0) * dots.astype(f)


def scores_emulate(dots, wn, xn):
    return -np.sqrt(np.maximum(d2_emulate(dots, wn, xn), np.float32(0.0)))


def ce_fwd_emulate(dots, wn, xn, ids):
    f = np.float32
    s = scores_emulate(dots, wn, xn)
    mx = s.max(1, keepdims=True)
    S = np.exp(s - mx).sum(1, keepdims=True, dtype=f)
    lse = (mx + np.log(S))[:, 0]
    return lse, lse - s[np.arange(s.shape[0]), ids]


def ce_bwd_emulate(dots, wn, xn, ids, lse, g):
    """-> G [N, V] (d_dots = -2 G), d_xn, d_wn"""
    f = np.float32
    s = scores_emulate(dots, wn, xn)
    oh = np.zeros_like(s)
    oh[np.arange(s.shape[0]), ids] = f(1.0)
    dl = g.astype(f)[:, None] * (np.exp(s - lse.astype(f)[:, None]) - oh)
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.where(s < 0, dl / (f(2.0) * s), f(0.0)).astype(f)
    return G, G.sum(1, dtype=f), G.sum(0, dtype=f)
