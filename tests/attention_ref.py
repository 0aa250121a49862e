"""Float64 reference of softmax attention (forward and analytic gradients) with the per-element error bounds the attention parity matrix
asserts, the stress inputs it runs on, and a float64 emulation of where the streaming kernels round.  Imported by
tests/test_attention_matrix_gpu.py and tests/test_attention_bound_cpu.py; not a conftest.  CPU only (torch).

Operands are [n, L, dh] (n = batch x heads) and already rounded to bf16.  With dropout, `keep` is bool [n, L, L] and Pd = P keep / (1 - p):

    S = scale q k^T,  P = softmax(S),  O = Pd v,  lse2 = log2(e) logsumexp(S)
    dV = Pd^T dO,  dPd = dO v^T,  dP = dPd keep / (1 - p),  D = rowsum(P dP) = rowsum(dO O),  dS = P (dP - D)
    dQ = scale dS k,  dK = scale dS^T q

Bounds (|got - ref| <= atol + 2^-8 |ref| for the bf16 outputs): the kernels convert P (un-normalised, then divided by an fp32 sum) and dS
to bf16 in registers before the second product, and form D from the bf16 O.  One bf16 rounding is 2^-9 relative; EPS = 2^-8 covers the
rounded factor and the normaliser / the second rounded factor:

    O[i,d]   EPS sum_j Pd[i,j] |v[j,d]|
    dV[j,d]  EPS sum_i Pd[i,j] |dO[i,d]|
    dQ[i,d]  scale (EPS sum_j |dS[i,j]| |k[j,d]| + dD[i] sum_j P[i,j] |k[j,d]|),  dD[i] = EPS sum_d |dO[i,d] O[i,d]|  (D's error enters dS as P dD)
    dK[j,d]  scale (EPS sum_i |dS[i,j]| |q[i,d]| + sum_i dD[i] P[i,j] |q[i,d]|)
    D[i]     against sum_d dO[i,d] O_given[i,d] (1 - p), O_given the bf16 rows the kernel reads: atol dh 2^-24 sum_d |dO O_given|, rtol 2^-22
    lse2[i]  atol log2(e) 2^-24 (L + dh scale |q_i| max_j |k_j|) (the fp32 sum of L terms; the fp32 score accumulation), rtol 2^-22"""
import math

import torch

LOG2E = math.log2(math.e)
EPS = 2.0 ** -8
RTOL_F32 = 2.0 ** -22


def bf16(x):
    """x rounded to bf16, as float64"""
    return x.float().bfloat16().double()


def f32(x):
    return x.float().double()


def _chunk(L):
    return max(1, (1 << 23) // (L * L))


def reference(q, k, v, scale, keep=None, p=0.0, dO=None, chained=False):
    """-> dict of float64 tensors: ctx, lse2 (+ D, dq, dk, dv with dO) and `<name>_atol`; o_given / lse2_given are the forward's results
    rounded to their storage types (bf16 / fp32) - what an isolated backward case feeds the kernels.  `keep` may be a callable
    (first, last) -> bool [last - first, L, L], so that no [n, L, L] tensor is ever held; the work goes in chunks of (batch, head)s.
    chained: the bounds of a backward that reads the forward KERNEL's O and lse2 instead of the reference's rounded ones: O is then within
    the forward's tolerance of the exact rows, not within one rounding, so dD[i] = sum_d |dO[i,d]| (atol_ctx[i,d] + EPS |O[i,d]|); lse2's
    error e scales every P by 2^e, so ln 2 x (lse2's tolerance) joins EPS in the dS and Pd terms"""
    n, L, dh = q.shape
    out = {}
    for a in range(0, n, _chunk(L)):
        b = min(n, a + _chunk(L))
        kp = None if keep is None else (keep(a, b) if callable(keep) else keep[a:b])
        part = _reference(q[a:b].double(), k[a:b].double(), v[a:b].double(), scale, kp, p, None if dO is None else dO[a:b].double(), chained)
        for name, t in part.items():
            out.setdefault(name, []).append(t)
    return {name: torch.cat(ts) for name, ts in out.items()}


def _reference(q, k, v, scale, keep, p, dO, chained=False):
    n, L, dh = q.shape
    P = (q @ k.transpose(1, 2)).mul_(scale)             # (S, E and P share one [n, L, L] buffer)
    m = P.max(-1, keepdim=True).values
    P.sub_(m).exp_()
    l = P.sum(-1, keepdim=True)
    P.div_(l)
    if keep is None:
        Pd = P
    elif dO is None:
        Pd = P.mul_(keep).mul_(1.0 / (1.0 - p))         # (forward only: P itself is not needed again)
    else:
        Pd = P * keep / (1.0 - p)
    r = {"ctx": Pd @ v, "ctx_atol": EPS * (Pd @ v.abs()), "lse2": LOG2E * (m + torch.log(l)).squeeze(-1)}
    r["lse2_atol"] = LOG2E * 2.0 ** -24 * (L + dh * scale * q.norm(dim=-1) * k.norm(dim=-1).max(-1, keepdim=True).values)
    r["o_given"], r["lse2_given"] = bf16(r["ctx"]), f32(r["lse2"])
    if dO is None:
        return r
    O = r["ctx"]
    dP = dO @ v.transpose(1, 2)
    if keep is not None:
        dP = dP * keep / (1.0 - p)
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - D)
    del dP
    dD = EPS * (dO * O).abs().sum(-1, keepdim=True)
    eps = EPS
    if chained:
        dD = (dO.abs() * (r["ctx_atol"] + EPS * O.abs())).sum(-1, keepdim=True)
        eps = EPS + math.log(2.0) * float((r["lse2_atol"] + RTOL_F32 * r["lse2"].abs()).max())
    r["dq"] = scale * (dS @ k)
    r["dk"] = scale * (dS.transpose(1, 2) @ q)
    r["dv"] = Pd.transpose(1, 2) @ dO
    aS = dS.abs()
    r["dq_atol"] = scale * (eps * (aS @ k.abs()) + dD * (P @ k.abs()))
    r["dk_atol"] = scale * (eps * (aS.transpose(1, 2) @ q.abs()) + (dD * P).transpose(1, 2) @ q.abs())
    r["dv_atol"] = eps * (Pd.transpose(1, 2) @ dO.abs())
    og = dO * r["o_given"]
    r["D"] = og.sum(-1) * (1.0 - p)
    r["D_atol"] = dh * 2.0 ** -24 * og.abs().sum(-1)
    return r


def emulate(q, k, v, scale, keep=None, p=0.0, dO=None):
    """the same quantities in float64 arithmetic that rounds exactly where the streaming kernels do: the softmax sum and lse2 to fp32, the
    un-normalised probabilities (forward), P / (1 - p) keep and dS (backward) to bf16 before the second product, D from the bf16 O, every
    output to its storage type.  The backward reads the REFERENCE's O and lse2 rounded to storage, as the isolated matrix cases do"""
    q, k, v = q.double(), k.double(), v.double()
    n, L, dh = q.shape
    ref = _reference(q, k, v, scale, keep, p, None)
    S = scale * (q @ k.transpose(1, 2))
    m = S.max(-1, keepdim=True).values
    E = torch.exp(S - m)
    l = f32(E.sum(-1, keepdim=True))
    Eb = bf16(E if keep is None else E * keep)
    r = {"ctx": bf16((Eb @ v) * (1.0 / (1.0 - p)) / l), "lse2": f32(LOG2E * (m + torch.log(l)).squeeze(-1))}
    if dO is None:
        return r
    dO = dO.double()
    Pr = torch.exp2(LOG2E * S - ref["lse2_given"].unsqueeze(-1)) / (1.0 - p)          # P / (1 - p), from the stored lse2
    D = f32((dO * ref["o_given"]).sum(-1, keepdim=True)) * (1.0 - p)
    dP = dO @ v.transpose(1, 2)
    if keep is not None:
        dP = dP * keep
    dS = bf16(Pr * (dP - D))
    Pb = bf16(Pr if keep is None else Pr * keep)
    r["D"] = f32(D.squeeze(-1))
    r["dq"] = bf16(scale * (dS @ k))
    r["dk"] = bf16(scale * (dS.transpose(1, 2) @ q))
    r["dv"] = bf16(Pb.transpose(1, 2) @ dO)
    return r


def ratios(got, ref, names):
    """{name: worst |got - ref| / (atol + rtol |ref|)} over every element (bf16 outputs: rtol EPS; D and lse2: RTOL_F32)"""
    out = {}
    for name in names:
        rtol = RTOL_F32 if name in ("D", "lse2") else EPS
        tol = ref[name + "_atol"] + rtol * ref[name].abs()
        out[name] = float(((got[name].double() - ref[name]).abs() / tol).max())
    return out


def stress_inputs(B, nh, L, dh, seed, hot=(), pre=False):
    """-> (qkv, dctx, q, k, v, dO): bf16 q, k, v, dO [B nh, L, dh] and the same values token-major (qkv [B L, 3 H], dctx [B L, H]: what
    training passes), with the stress the kernels' softmax needs:
      * one key far above the rest late in the sequence (300) and one inside the last - possibly partial - tile (L - 3): running-max rescale;
      * (batch, head) 1: every score far below zero (the first tile's reference is a large negative number);
      * key L - 3 of every head aligned with query 17: that query's score beats its predecessors by far more than 2^8 in the log2 domain
        (the pre-scaled form re-bases);
      * (batch, head)s `hot`: key 5 - the first stage of the item - dominates.  The matrix names the second and third items a persistent
        block walks: a running maximum or sum that is not reset, or a stage left over from the previous item, then changes the result
        by far more than the tolerance.
    pre: the stored queries carry scale x log2(e) (rounded once more, as the QKV epilogue stores them); the reference then uses scale = ln 2"""
    H, n = nh * dh, B * nh
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, L, dh, generator=g) * 0.8 for _ in range(3))
    dO = (torch.randn(n, L, dh, generator=g) * 0.5).bfloat16()
    k *= 1.5
    k[:, 300] *= 4.0
    k[:, L - 3] = 40.0 * q[:, 17] / q[:, 17].norm(dim=-1, keepdim=True)
    if n > 1:
        q[1] = q[1].abs() + 2.0
        k[1] = -(k[1].abs() + 2.0)
    for bh in hot:
        k[bh, 5] = 30.0 * q[bh, 40] / q[bh, 40].norm(dim=-1, keepdim=True) + 2.0 * k[bh, 5]
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    if pre:
        q = (q.float() * (LOG2E / math.sqrt(dh))).bfloat16()
    tok = lambda x: x.view(B, nh, L, dh).permute(0, 2, 1, 3).reshape(B * L, H)  # noqa: E731
    return torch.cat([tok(q), tok(k), tok(v)], dim=1), tok(dO), q, k, v, dO
