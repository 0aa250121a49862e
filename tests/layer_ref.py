"""Float64 reference of ONE encoder layer of the training step (csrc/train_layer.hip: mh_train_layer_fwd / mh_train_layer_bwd - a HF
BertLayer in train mode, forward and backward), in the stage order of that file's header comment.  Imported by
tests/test_train_layer_matrix_gpu.py (the two calls against it) and tests/test_train_layer_bound_cpu.py (the backward tolerance sees
wiring errors and admits a correct implementation); not a conftest.  CPU only (torch float64, numpy for the LayerNorm backward).

Every kernel the two calls launch has its own per-element parity case (tests/test_gemm_matrix_gpu.py, test_attention_matrix_gpu.py,
test_train_matrix_gpu.py); what is checked here is the composition: which buffer, which dropout site, which residual, which offset of
`grads`, which split slices.  Nothing is restated that exists: the attention stage is attention_ref.reference / emulate, the LayerNorm
backward train_ref.ln_bwd / ln_bwd_emulate, the dense bounds acc_bound + RTOL_BF16 |ref| and the activation allowances of run_dense, the
dense keep flags gemm_census.dense_keep.

* forward_stages: every buffer the forward leaves behind against the float64 value of THAT stage, computed from the stage's inputs as
  the kernel stored them (x and the kernel's own earlier buffers) - per element, with the bound the kernel's own matrix uses.
* backward: the analytic float64 gradients (dx and the twelve blocks of `grads`) from the saved forward tensors.
* backward_emulated: the same in float64 arithmetic that rounds exactly where mh_train_layer_bwd stores or converts.  The backward is a
  chain of four to five dense products; a worst-case bound carried through it exceeds the signal, so the kernels are held against the
  emulation's own error (`errors`, `margins`):  e_rms(kernel) <= 2 e_rms(emulated) + 2^-22,  e_max(kernel) <= 3 e_max(emulated) + 2^-22
  per output tensor, e_rms = |got - ref|_2 / |ref|_2, e_max = max |got - ref| / max |ref|.  The emulation is one realisation of the same
  roundings at the same places; over tensors of 512 elements and more two realisations agree in RMS to tens of percent and in maximum
  to within a factor of two.
* MUTANTS: backward_emulated with one wiring error each; the CPU test shows that the margins see every one of them.

Tensors are token-major [N, cols] on the host whatever the device layout (rows or K32 panels); N = B L."""
import functools
import math

import numpy as np
import torch

import attention_ref as ar
import train_ref as tr
from test_gemm_matrix_gpu import ACT_ATOL, GELU, RTOL_BF16, acc_bound, act_ref, gelu_grad

H = 512
LN_EPS = 1e-12
GRAD_NAMES = ("dWqkv", "dbqkv", "dWao", "dbao", "dW1", "db1", "dW2", "db2", "dln1_g", "dln1_b", "dln2_g", "dln2_b")
OUTPUTS = ("dx",) + GRAD_NAMES
FORWARD_BUFFERS = ("qkv", "vt", "ctx", "lse", "pre1", "x1", "g", "dact", "pre2", "y")
RMS_FACTOR, MAX_FACTOR, FLOOR = 2.0, 3.0, 2.0 ** -22


def grad_sizes(F):
    """floats of the twelve blocks of `grads`, in order (include/musehip.h: mh_train_layer)"""
    return [3 * H * H, 3 * H, H * H, H, F * H, F, H * F, H, H, H, H, H]


# ------------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=4)
def layer_inputs(B, L, F, seed=0):
    """x: bf16 rows that look like a LayerNorm output (O(1), with a per-row offset as in train_ref.ln_inputs); weights 1.5 / sqrt(K), biases
    0.3, gains 1 +- 0.2, shifts 0.1, dy 0.5 N(0, 1) in bf16.  Weights are bf16 values [out, in] (the device operands are panels of these and
    of their transposes, built on the host by the caller); vectors are fp32"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + L + F)
    N = B * L
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    off = (torch.rand(N, 1, generator=g) * 2 - 1) * 0.5
    w = lambda o, i: (rn(o, i) * (1.5 / math.sqrt(i))).bfloat16()  # noqa: E731
    return {"x": (rn(N, H) + off).bfloat16(), "dy": (0.5 * rn(N, H)).bfloat16(),
            "Wqkv": w(3 * H, H), "Wao": w(H, H), "W1": w(F, H), "W2": w(H, F),
            "bqkv": 0.3 * rn(3 * H), "bao": 0.3 * rn(H), "b1": 0.3 * rn(F), "b2": 0.3 * rn(H),
            "ln1_g": 1 + 0.2 * rn(H), "ln1_b": 0.1 * rn(H), "ln2_g": 1 + 0.2 * rn(H), "ln2_b": 0.1 * rn(H)}


def no_masks():
    return {"attn": (None, 0.0), "ao": (None, 0.0), "ffn": (None, 0.0)}


def random_masks(B, L, nh, p, seed):
    """keep flags of the three sites (attn [B nh, L, L], ao / ffn [N, H]) for p = (p_attn, p_ao, p_ffn); a site with p = 0 is off"""
    g = torch.Generator().manual_seed(seed)
    shapes = {"attn": (B * nh, L, L), "ao": (B * L, H), "ffn": (B * L, H)}
    return {s: ((torch.rand(*shapes[s], generator=g) >= ps) if ps > 0 else None, float(np.float32(ps))) for s, ps in zip(("attn", "ao", "ffn"), p)}


# ------------------------------------------------------------------------------------------------------------------------ helpers
def heads(x, B, L, nh):
    """token-major [B L, nh dh] -> [B nh, L, dh]"""
    return x.reshape(B, L, nh, -1).permute(0, 2, 1, 3).reshape(B * nh, L, -1)


def tokens(x, B, L, nh):
    """[B nh, L, dh] -> token-major [B L, nh dh]"""
    return x.reshape(B, nh, L, -1).permute(0, 2, 1, 3).reshape(B * L, -1)


def _d(x):
    return x.double()


def _rscale(p):
    """1 / (1 - p) as the kernels form it (fp32)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _drop(v, site):
    keep, p = site
    if keep is None:
        return v
    return torch.where(keep, v / (1.0 - p), torch.zeros_like(v))


def _layer_norm(pre, gamma, beta):
    v = _d(pre)
    mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    return (v - mu) / torch.sqrt(var + LN_EPS) * _d(gamma) + _d(beta)


def _shape(saved, nh):
    N = saved["x"].shape[0]
    L = saved["lse"].shape[1]
    return N // L, L, N


# ------------------------------------------------------------------------------------------------------------------------ forward
def forward_stages(saved, w, masks, nh):
    """{buffer: (ref, atol, rtol)} - |got - ref| <= atol + rtol |ref| element by element; each stage from the STORED inputs of that stage"""
    B, L, N = _shape(saved, nh)
    dh, F = H // nh, w["W1"].shape[0]
    scale = 1.0 / math.sqrt(dh)
    out = {}
    x = saved["x"]
    # qkv = x Wqkv^T + b (rows): dense
    out["qkv"] = (_d(x) @ _d(w["Wqkv"]).T + _d(w["bqkv"]), acc_bound(x, w["Wqkv"], H), RTOL_BF16)
    # vt: head_permute mode 4 of the stored V columns - exact, with its 256 zeroed tail elements
    v_np = saved["qkv"][:, 2 * H:].float().numpy()
    vt = np.concatenate([tr.head_permute(v_np, B, L, nh, dh, 4).reshape(-1), np.zeros(256, np.float32)])
    out["vt"] = (torch.from_numpy(vt).double(), 0.0, 0.0)
    # attention on the stored q | k | v
    q, k, v = (heads(saved["qkv"][:, i * H:(i + 1) * H], B, L, nh) for i in range(3))
    keep, p = masks["attn"]
    r = ar.reference(q, k, v, scale, keep, p)
    out["ctx"] = (tokens(r["ctx"], B, L, nh), tokens(r["ctx_atol"], B, L, nh), ar.EPS)
    out["lse"] = (r["lse2"], r["lse2_atol"], ar.RTOL_F32)
    # pre = drop(A W^T + b) + residual (rows), then LayerNorm of the STORED bf16 rows (2^-16: run_dense)
    for pre, ln, A, W, b, res, site, gm, bt in (("pre1", "x1", saved["ctx"], w["Wao"], w["bao"], x, masks["ao"], w["ln1_g"], w["ln1_b"]),
                                                ("pre2", "y", saved["g"], w["W2"], w["b2"], saved["x1"], masks["ffn"], w["ln2_g"], w["ln2_b"])):
        val = _drop(_d(A) @ _d(W).T + _d(b), site) + _d(res)
        tol = acc_bound(A, W, A.shape[1]) / (1.0 - site[1])
        out[pre] = (val, tol, RTOL_BF16)
        out[ln] = (_layer_norm(saved[pre], gm, bt), 2.0 ** -16, RTOL_BF16)
    # g = gelu(x1 W1^T + b), dact = gelu'(.): the allowances of run_dense
    eb = acc_bound(saved["x1"], w["W1"], H)
    z = _d(saved["x1"]) @ _d(w["W1"]).T + _d(w["b1"])
    out["g"] = (act_ref(z, GELU), eb + ACT_ATOL, RTOL_BF16)
    out["dact"] = (gelu_grad(z), 2e-4 + 1e-3 * (z.abs() < 1e-2) + 0.4 * eb, RTOL_BF16)
    return out


def forward_saved(inp, masks, nh, B, L):
    """the forward's saved tensors without a device: float64 arithmetic rounded to each buffer's storage type (what the CPU test feeds the
    backward references)"""
    R = ar.bf16
    x = inp["x"]
    dh = H // nh
    s = {"x": x}
    s["qkv"] = R(_d(x) @ _d(inp["Wqkv"]).T + _d(inp["bqkv"])).bfloat16()
    q, k, v = (heads(s["qkv"][:, i * H:(i + 1) * H], B, L, nh) for i in range(3))
    keep, p = masks["attn"]
    e = ar.emulate(q, k, v, 1.0 / math.sqrt(dh), keep, p)
    s["ctx"], s["lse"] = tokens(e["ctx"], B, L, nh).bfloat16(), e["lse2"].float()
    s["pre1"] = R(_drop(_d(s["ctx"]) @ _d(inp["Wao"]).T + _d(inp["bao"]), masks["ao"]) + _d(x)).bfloat16()
    s["x1"] = R(_layer_norm(s["pre1"], inp["ln1_g"], inp["ln1_b"])).bfloat16()
    z = _d(s["x1"]) @ _d(inp["W1"]).T + _d(inp["b1"])
    s["g"], s["dact"] = R(act_ref(z, GELU)).bfloat16(), R(gelu_grad(z)).bfloat16()
    s["pre2"] = R(_drop(_d(s["g"]) @ _d(inp["W2"]).T + _d(inp["b2"]), masks["ffn"]) + _d(s["x1"])).bfloat16()
    s["y"] = R(_layer_norm(s["pre2"], inp["ln2_g"], inp["ln2_b"])).bfloat16()
    return s


# ------------------------------------------------------------------------------------------------------------------------ backward
def _ln_bwd64(pre, dy, gamma):
    r = tr.ln_bwd(pre.float().numpy(), dy.float().numpy() if dy.dtype != torch.float64 else dy.numpy(), gamma.float().numpy(), LN_EPS, tr.BF16)
    return tuple(torch.from_numpy(np.asarray(r[n][0], dtype=np.float64)) for n in ("dx", "dgamma", "dbeta"))


def _ln_bwd_rounded(pre, g_in, gamma):
    """ln_bwd_kernel's formula (csrc/train.hip) in float64 with every fp32 register value it forms rounded to fp32: the mean (:315), the
    deviations and rstd (:322-324), xhat and dy gamma (:334-335), the products that enter the row and column sums (:336-338), s1 and s2
    (:343), dx before its bf16 store (:350).  dln2 has NO bf16 rounding upstream (its inputs are the stored pre2 and dy), so these are
    the roundings that set its error: without them the emulation's dln2_g error was 2e-8 and a float32 realisation's 4e-7"""
    F = ar.f32
    x, dy, gm = _d(pre), _d(g_in), _d(gamma)
    n = x.shape[1]
    mean = F(x.sum(1, keepdim=True) / n)
    d = F(x - mean)
    rstd = F(1.0 / torch.sqrt(F(F(d * d).sum(1, keepdim=True) / n + float(np.float32(LN_EPS)))))
    xh, dg = F(d * rstd), F(dy * gm)
    s1, s2 = F(dg.sum(1, keepdim=True) / n), F(F(dg * xh).sum(1, keepdim=True) / n)
    dx = F(rstd * F(F(dg - s1) - F(xh * s2)))
    return dx, ln_column_sum(F(dy * xh), F), ln_column_sum(dy, F)


def ln_column_sum(terms, rnd):
    """sum over the rows of terms [N, H] in the order of ln_bwd_kernel and colsum_final_kernel, every partial sum through `rnd` (round to
    fp32; the identity for float32 tensors): wave w of block b adds rows 4 b + w, + 4 P, ... in a register (train.hip:337-338), the block
    writes (w0 + w1) + (w2 + w3) (:373), lane l of the fold adds partials l, l + 16, ... in order and the 16 lanes are added in order
    (:191-203); P = min(N / 4, 1024) blocks (train_layer.hip:43).  A plain sequential fp32 sum of 512 rows is off by 4e-7 of the result -
    more than the 2^-22 the tolerance leaves for a gradient that no bf16 rounding precedes (dln2) - where this order stays below 1e-7"""
    N, cols = terms.shape
    assert N % 4 == 0
    P = min(N // 4, 1024)
    zero = lambda *s: torch.zeros(*s, cols, dtype=terms.dtype)  # noqa: E731
    t = torch.cat([terms, zero((-N) % (4 * P))]).reshape(-1, P, 4, cols)
    acc = zero(P, 4)
    for step in t:
        acc = rnd(acc + step)
    part = rnd(rnd(acc[:, 0] + acc[:, 1]) + rnd(acc[:, 2] + acc[:, 3]))
    part = torch.cat([part, zero((-P) % 16)]).reshape(-1, 16, cols)
    lanes = zero(16)
    for step in part:
        lanes = rnd(lanes + step)
    total = zero()
    for lane in lanes:
        total = rnd(total + lane)
    return total


def _ln_bwd_f32(pre, g_in, gamma):
    """the LayerNorm backward in float32 arithmetic: dx is train_ref.ln_bwd_emulate's, the column sums take ln_column_sum's order"""
    f = np.float32
    x, dy, gm = pre.float().numpy(), g_in.float().numpy(), gamma.float().numpy()
    dx = tr.ln_bwd_emulate(x, dy, gm, LN_EPS, tr.BF16)[0]
    d = x - x.sum(1, keepdims=True, dtype=f) / f(x.shape[1])
    xh = d * (f(1.0) / np.sqrt((d * d).sum(1, keepdims=True, dtype=f) / f(x.shape[1]) + f(LN_EPS)))
    same = lambda v: v  # noqa: E731
    return (torch.from_numpy(dx).double(), ln_column_sum(torch.from_numpy(dy * xh), same).double(),
            ln_column_sum(torch.from_numpy(dy), same).double())


def backward(saved, w, masks, dy, nh):
    """the analytic float64 backward from the saved forward tensors: {"dx", *GRAD_NAMES}.  P is recomputed in float64 from the stored
    qkv (attention_ref.reference, chained)"""
    B, L, N = _shape(saved, nh)
    dh = H // nh
    o = {}
    r2, o["dln2_g"], o["dln2_b"] = _ln_bwd64(saved["pre2"], dy, w["ln2_g"])
    m2 = _drop(r2, masks["ffn"])
    o["dW2"], o["db2"] = m2.T @ _d(saved["g"]), m2.sum(0)
    d1 = (m2 @ _d(w["W2"])) * _d(saved["dact"])
    o["dW1"], o["db1"] = d1.T @ _d(saved["x1"]), d1.sum(0)
    t = d1 @ _d(w["W1"]) + r2
    r1, o["dln1_g"], o["dln1_b"] = _ln_bwd64(saved["pre1"], t, w["ln1_g"])
    m1 = _drop(r1, masks["ao"])
    o["dWao"], o["dbao"] = m1.T @ _d(saved["ctx"]), m1.sum(0)
    dctx = m1 @ _d(w["Wao"])
    q, k, v = (heads(saved["qkv"][:, i * H:(i + 1) * H], B, L, nh) for i in range(3))
    keep, p = masks["attn"]
    a = ar.reference(q, k, v, 1.0 / math.sqrt(dh), keep, p, heads(dctx, B, L, nh), chained=True)
    dqkv = torch.cat([tokens(a[n], B, L, nh) for n in ("dq", "dk", "dv")], dim=1)
    o["dWqkv"], o["dbqkv"] = dqkv.T @ _d(saved["x"]), dqkv.sum(0)
    o["dx"] = dqkv @ _d(w["Wqkv"]) + r1
    return o


def attention_bwd_emulated(q, k, v, scale, keep, p, dO, o_given, lse2_given, f32=False, mask_dp=True):
    """attention_ref.emulate's backward lines with O and lse2 GIVEN (the layer's backward reads the forward kernel's ctx and lse, not the
    reference's): P / (1 - p) from the stored lse2, D in fp32 from the bf16 O, dS and P keep / (1 - p) to bf16 before the second products,
    dq / dk / dv to bf16.  With the reference's rounded O and lse2 it IS attention_ref.emulate (tests/test_train_layer_bound_cpu.py).
    f32: the sums in float32.  mask_dp = False: mutant (e)"""
    mm = (lambda a, b: (a.float() @ b.float()).double()) if f32 else (lambda a, b: a @ b)
    n, L, dh = q.shape
    step = max(1, ar._chunk(L) // 2)
    out = {"dq": [], "dk": [], "dv": []}
    for a in range(0, n, step):
        sl = slice(a, min(n, a + step))
        qq, kk, vv, dd, oo = (_d(t[sl]) for t in (q, k, v, dO, o_given))
        kp = None if keep is None else keep[sl]
        S = scale * mm(qq, kk.transpose(1, 2))
        Pr = torch.exp2(ar.LOG2E * S - _d(lse2_given[sl]).unsqueeze(-1)) / (1.0 - p)
        prod = dd * oo
        D = ar.f32(prod.float().sum(-1, keepdim=True).double() if f32 else prod.sum(-1, keepdim=True)) * (1.0 - p)
        dP = mm(dd, vv.transpose(1, 2))
        if kp is not None and mask_dp:
            dP = dP * kp
        dS = ar.bf16(Pr * (dP - D))
        Pb = ar.bf16(Pr if kp is None else Pr * kp)
        out["dq"].append(ar.bf16(scale * mm(dS, kk)))
        out["dk"].append(ar.bf16(scale * mm(dS.transpose(1, 2), qq)))
        out["dv"].append(ar.bf16(mm(Pb.transpose(1, 2), dd)))
    return {n_: torch.cat(ts) for n_, ts in out.items()}


def split_rows(N, S):
    """token rows [first, last) of the S split-K slices of a weight gradient over N tokens: N / 32 K-steps, the slices differ by at most
    one step (csrc/gemm_dw.hip)"""
    steps = N // 32
    edges = [32 * ((i * steps) // S) for i in range(S + 1)]
    return list(zip(edges[:-1], edges[1:]))


def backward_emulated(saved, w, masks, dy, nh, f32=False, mutant=None, splits=1):
    """`backward` in float64 arithmetic, rounded where mh_train_layer_bwd stores or converts (line numbers: csrc/train_layer.hip; the
    kernels behind them round once, from an fp32 accumulator).  f32: every fp32 sum taken in float32 (GEMM accumulations, the LayerNorm
    backward's reductions, column sums, D) - a second realisation of the same roundings.  mutant: a key of MUTANTS.  splits: the
    split-K slices of dWqkv (only mutant (i) reads it)"""
    B, L, N = _shape(saved, nh)
    dh = H // nh
    R, F32 = ar.bf16, ar.f32
    mm = (lambda a, b: (a.float() @ b.float()).double()) if f32 else (lambda a, b: a @ b)
    colsum = (lambda a: a.float().sum(0).double()) if f32 else (lambda a: a.sum(0))

    def ln(pre, g_in, gamma):
        return _ln_bwd_f32(pre, g_in, gamma) if f32 else _ln_bwd_rounded(pre, g_in, gamma)

    def dropped(r, site, scale_on=True):
        keep, p = site
        if keep is None:
            return r
        return R(torch.where(keep, r * (_rscale(p) if scale_on else 1.0), torch.zeros_like(r)))

    o = {}
    # :229 ln_bwd(pre2, dy) -> r (rows, bf16), m = keep o r / (1 - p) of the ROUNDED r (panels, bf16); dln2 partials folded in fp32
    r2, dg2, db2 = ln(saved["pre2"], dy, w["ln2_g"])
    r2 = R(r2)
    m2 = dropped(r2, masks["ao"] if mutant == "a" else masks["ffn"])
    o["dln2_g"], o["dln2_b"] = F32(dg2), F32(db2)
    # :230 dW2 | db2 = m2^T g, fp32
    o["dW2"], o["db2"] = F32(mm(m2.T, _d(saved["g"]))), F32(colsum(r2 if mutant == "f" else m2))
    # :231-236 d1 = (m W2) o gelu' -> bf16 panels
    d1 = R(mm(m2, _d(w["W2"])) * _d(saved["dact"]))
    # :237 dW1 | db1 = d1^T x1, fp32
    o["dW1"], o["db1"] = F32(mm(d1.T, _d(saved["pre1"] if mutant == "g" else saved["x1"]))), F32(colsum(d1))
    # :238-243 t = d1 W1 + r -> bf16 rows
    t = R(mm(d1, _d(w["W1"])) + (0.0 if mutant == "c" else r2))
    # :244 ln_bwd(pre1, t) -> r1 rows, m1 panels (bf16), dln1 fp32
    r1, dg1, db1 = ln(saved["pre1"], t, w["ln1_g"])
    r1 = R(r1)
    m1 = dropped(r1, masks["ao"], scale_on=mutant != "b")
    o["dln1_g"], o["dln1_b"] = F32(dg1), F32(db1)
    # :245 dWao | dbao = m1^T ctx, fp32
    o["dWao"], o["dbao"] = F32(mm(m1.T, _d(saved["ctx"]))), F32(colsum(m1))
    # :246-250 d(ctx) = m Wao -> bf16 rows
    dctx = R(mm(m1, _d(w["Wao"])))
    # :251-258 attention backward on the stored qkv, ctx (bf16) and lse: D fp32, P and dS bf16 inside, dqkv bf16 panels
    q, k, v = (heads(saved["qkv"][:, i * H:(i + 1) * H], B, L, nh) for i in range(3))
    keep, p = masks["attn"]
    a = attention_bwd_emulated(q, k, v, 1.0 / math.sqrt(dh), keep, p, heads(dctx, B, L, nh), heads(saved["ctx"], B, L, nh),
                               saved["lse"], f32=f32, mask_dp=mutant != "e")
    dqkv = torch.cat([tokens(a[n], B, L, nh) for n in ("dq", "dk", "dv")], dim=1)
    # :259 dWqkv | dbqkv = dqkv^T x, fp32 (split-K slices folded in fixed order)
    dq_w = dqkv
    if mutant == "i":
        assert splits > 1, "mutant (i) needs a split weight gradient"
        first, last = split_rows(N, splits)[-1]
        dq_w = dqkv.clone()
        dq_w[first:last] = 0.0
    o["dWqkv"], o["dbqkv"] = F32(mm(dq_w.T, _d(saved["x"]))), F32(colsum(dq_w))
    # :260-265 dx = dqkv Wqkv + r -> bf16 rows
    o["dx"] = R(mm(dqkv, _d(w["Wqkv"])) + (0.0 if mutant == "d" else r1))
    if mutant == "h":
        o["dln1_g"], o["dln1_b"], o["dln2_g"], o["dln2_b"] = o["dln2_g"], o["dln2_b"], o["dln1_g"], o["dln1_b"]
    return o


# name -> (what is wired wrongly, needs dropout, needs splits > 1)
MUTANTS = {
    "a": ("LN2's dense-branch mask taken from the attention-output site", True, False),
    "b": ("1 / (1 - p) missing on m1", True, False),
    "c": ("r2 not added into t", False, False),
    "d": ("r1 not added into dx", False, False),
    "e": ("the attention keep mask not applied to dP", True, False),
    "f": ("db2 summed from r2 instead of m2", True, False),
    "g": ("dW1 formed with pre1 instead of x1", False, False),
    "h": ("the dln1 and dln2 blocks of grads exchanged", False, False),
    "i": ("one split slice of dWqkv left out", False, True),
}


# ------------------------------------------------------------------------------------------------------------------------ the tolerance
def errors(got, ref):
    """{tensor: (e_rms, e_max)} - normalised per TENSOR (dbqkv as one tensor of 3 H elements: its key block is zero in exact arithmetic)"""
    out = {}
    for n in OUTPUTS:
        g, r = _d(got[n]).reshape(-1), _d(ref[n]).reshape(-1)
        assert g.shape == r.shape, (n, g.shape, r.shape)
        d = g - r
        out[n] = (float(d.norm() / r.norm()), float(d.abs().max() / r.abs().max()))
    return out


def margins(e_got, e_emu):
    """{tensor: (e_rms(got) / (2 e_rms(emu) + 2^-22), e_max(got) / (3 e_max(emu) + 2^-22))}: inside the tolerance when both are <= 1"""
    return {n: (e_got[n][0] / (RMS_FACTOR * e_emu[n][0] + FLOOR), e_got[n][1] / (MAX_FACTOR * e_emu[n][1] + FLOOR)) for n in OUTPUTS}


def worst(m):
    """(largest ratio, its tensor)"""
    return max((max(v), n) for n, v in m.items())


def table(case, e_got, e_emu, label="kernel"):
    """the lines of profiles/train_layer_matrix.txt for one case"""
    m = margins(e_got, e_emu)
    return ["LAYER-BWD %-22s %-7s emu e_rms %.3e e_max %.3e | %s e_rms %.3e e_max %.3e | ratio rms %.2f max %.2f | of margin %.2f %.2f"
            % (case, n, e_emu[n][0], e_emu[n][1], label, e_got[n][0], e_got[n][1], e_got[n][0] / max(e_emu[n][0], 1e-300),
               e_got[n][1] / max(e_emu[n][1], 1e-300), m[n][0], m[n][1]) for n in OUTPUTS]
