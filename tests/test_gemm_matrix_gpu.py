"""Parity matrix: every GEMM variant the product launches (tests/test_gemm_census_gpu.py: PARITY) against a float64 reference on the CPU,
element by element, at the shapes where tiling code goes wrong:

* ragged: M not a multiple of the tile's rows, N a multiple of 8 (32 for a K32-panel output) but not of the tile's columns, K an odd
  multiple of 32 (the big-tile kernels step K by 32 and pair steps);
* multi-tile: the persistent kernels launch at most `slots` = CUs x blocks per CU blocks; tiles = 2 slots + r (0 < r < slots) makes every
  block walk two or three tiles, so the next tile's stages land in the ring while this tile's epilogue runs, and the last tile is ragged;
* row window: K32-panel operands that are a row window of larger panel buffers (lda > M, first row > 0).

Operands are rounded to their storage type first (bf16, or the split modes' fp32 input), the reference is float64.  Every output buffer
starts as NaN, so a tile that is never written fails, and whatever lies outside the output's rows / columns must still be NaN afterwards.
Tolerances are per element: |got - ref| <= atol_i + rtol |ref_i|, with atol_i from the accumulation (see `acc_bound`)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import gemm_census as gc

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import MH_BF16, MH_BF16X3, MH_F16X3, MH_F32, check, current_stream, lib  # noqa: E402

DEV = "cuda"
NONE, TANH, GELU, SILU, DERIV = 0, 1, 2, 3, 4
# bf16 output: round-to-nearest leaves at most half an ulp = 2^-9 |v| (relative); 2^-8 allows the value before rounding to sit anywhere
# within the accumulation bound of the reference (atol) and still round the same way or to the neighbour
RTOL_BF16 = 2.0 ** -8
# fp32 output: the result is the fp32 sum itself (no output rounding beyond 2^-24 relative); what remains is the accumulation (atol)
RTOL_F32 = 2.0 ** -22
# the epilogues' fast GELU / tanh / SiLU (csrc/common.h: gelu_erf_fast8, apply_act) are within 1.1e-4 absolute of the exact function;
# rounded up to 2e-4
ACT_ATOL = 2e-4
# split modes: max |err| / rms(ref) of a length-512 product sum (tests/test_split_gpu.py: GEMM_TOL), applied per element as atol = GEMM_TOL
# rms(ref) (the existing bound) + GEMM_TOL |ref_i|
GEMM_TOL = {MH_BF16X3: 8e-5, MH_F16X3: 1.2e-5}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def multi_rows(tile_m, tiles_n, per_cu):
    """M for a persistent launch of ceil(M / tile_m) x tiles_n tiles = 2 slots + r with 0 < r < slots, the last row tile ragged"""
    slots = _cus() * per_cu
    target = 2 * slots + slots // 8 + 1
    rows = -(-target // tiles_n)
    tiles = rows * tiles_n
    assert 2 * slots < tiles < 3 * slots, (tiles, slots)
    return rows * tile_m - 40


def acc_bound(A, W, K):
    """per-element bound of the fp32 accumulation error: K 2^-24 sum_k |a_k w_k| (the recursive-summation bound), with the sum bounded by
    |a| |w| (Cauchy-Schwarz: an outer product of row norms instead of a second matrix product)"""
    return K * 2.0 ** -24 * torch.outer(A.double().norm(dim=1), W.double().norm(dim=1))


@functools.lru_cache(maxsize=3)
def operands(M, N, K, seed):
    """bf16 A [M, K], W [N, K] and the float64 product A W^T (cached: several variants share a shape)"""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * 0.7).bfloat16()
    W = (torch.randn(N, K, generator=g) * (1.5 / math.sqrt(K))).bfloat16()
    z = A.double() @ W.double().T
    return A, W, z, acc_bound(A, W, K)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(name, got, ref, atol, rtol):
    got = got.double().cpu()
    ref = ref.double()
    assert bool(torch.isfinite(got).all()), "%s: %d elements never written (still NaN) or not finite" % (name, int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    if bool(bad.any()):
        i = int((err - tol).argmax())
        idx = np.unravel_index(i, tuple(ref.shape))
        pytest.fail("%s: %d of %d elements outside |got - ref| <= atol + %.3g |ref|; worst at %s: got %.6g ref %.6g (tol %.3g); first bad rows %s"
                    % (name, int(bad.sum()), bad.numel(), rtol, idx, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(tol.reshape(-1)[i]),
                       sorted(set(torch.nonzero(bad)[:, 0].tolist()))[:8] if bad.dim() > 1 else "-"))


# ------------------------------------------------------------------------------------------------------------------- layouts
class Operand:
    """a [rows, cols] bf16 operand on the device, row-major (pitch cols + 16) or as K32 panels [cols / 32][ld][32] whose rows start at
    row r0 of a larger buffer (window).  Inputs are padded with zeros; outputs (fill) start as NaN everywhere"""

    def __init__(self, x, panel, r0=0, extra=0, fill=None, dtype=torch.bfloat16):
        self.rows, self.cols = x.shape
        self.panel, self.r0 = panel, r0
        if panel:
            self.ld = r0 + self.rows + extra
            buf = torch.full((self.cols // 32, self.ld, 32), 0.0 if fill is None else float("nan"), dtype=dtype)
            if fill is None:
                buf[:, r0:r0 + self.rows] = x.to(dtype).reshape(self.rows, self.cols // 32, 32).permute(1, 0, 2)
            self.buf = buf.to(DEV)
            self.ptr = self.buf.data_ptr() + r0 * 32 * self.buf.element_size()
        else:
            self.ld = self.cols + (16 if extra else 0)
            buf = torch.full((self.rows + r0, self.ld), 0.0 if fill is None else float("nan"), dtype=dtype)
            if fill is None:
                buf[r0:, :self.cols] = x.to(dtype)
            self.buf = buf.to(DEV)
            self.ptr = self.buf.data_ptr() + r0 * self.ld * self.buf.element_size()

    def read(self):
        """the operand's [rows, cols] on the host; asserts that nothing outside its rows / columns was written"""
        b = self.buf.cpu()
        if self.panel:
            outside = torch.cat([b[:, :self.r0].reshape(-1), b[:, self.r0 + self.rows:].reshape(-1)])
            x = b[:, self.r0:self.r0 + self.rows].permute(1, 0, 2).reshape(self.rows, self.cols)
        else:
            outside = torch.cat([b[:self.r0].reshape(-1), b[self.r0:, self.cols:].reshape(-1)])
            x = b[self.r0:, :self.cols]
        assert bool(torch.isnan(outside.float()).all()), "written outside the output's rows / columns"
        return x


def out_operand(M, N, panel, window, dtype=torch.bfloat16):
    return Operand(torch.empty(M, N), panel, r0=64 if window else 0, extra=64 if window else 16, fill="nan", dtype=dtype)


def in_operand(x, panel, window):
    return Operand(x, panel, r0=96 if window else 0, extra=32 if window else 16)


# --------------------------------------------------------------------------------------------------- reference epilogue
def act_ref(z, act):
    if act == TANH:
        return torch.tanh(z)
    if act == GELU:
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))
    if act == SILU:
        return z * torch.sigmoid(z)
    return z


def gelu_grad(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-z * z / 2) / math.sqrt(2 * math.pi)


def run_dense(M, N, K, *, act=NONE, res=False, act_grad=0, pre_kind=None, drop=0.0, ln=False, out_f32=False, panels="", window=False,
              bias=True, seed=0):
    """one launch through mh_gemm_desc_launch (every bf16 dense launch of the training step and the engine's row-major ones): operands
    row-major or K32 panels per the letters of `panels` (a, w, o, r, p), then every output against the float64 reference"""
    A, W, z, eb = operands(M, N, K, seed)
    b = rnd(N, seed=seed + 1, scale=0.3) if bias else None
    pre = z + b.double() if bias else z.clone()
    R = None
    if act_grad == DERIV:
        R = torch.rand(M, N, generator=torch.Generator().manual_seed(seed + 2)).mul(1.1).bfloat16()     # gelu'(pre) lies in (-0.13, 1.13)
    elif act_grad:
        R = rnd(M, N, seed=seed + 2, scale=2.0).bfloat16()                                                # the pre-activation
    elif res or ln:
        R = rnd(M, N, seed=seed + 2).bfloat16()
    d = None
    if drop or ln:
        d = _lib.Dropout()
        d.p, d.seed, d.offset, d.mask = drop, 0x5DEECE66D ^ seed, (11 << 16) | (seed & 0xFFFF), None
    gamma, beta = (1 + 0.2 * rnd(N, seed=seed + 3), 0.1 * rnd(N, seed=seed + 4)) if ln else (None, None)
    Ao, Wo = in_operand(A, "a" in panels, window), in_operand(W, "w" in panels, window)
    Ro = in_operand(R, "r" in panels, window) if R is not None else None
    Oo = out_operand(M, N, "o" in panels, window, torch.float32 if out_f32 else torch.bfloat16)
    Po = out_operand(M, N, "p" in panels, window) if (pre_kind is not None or ln) else None
    bd = b.to(DEV) if bias else None
    gd, btd = (gamma.to(DEV), beta.to(DEV)) if ln else (None, None)
    desc = _lib.GemmDesc(A=Ao.ptr, lda=Ao.ld, a_panel=Ao.panel, W=Wo.ptr, ldw=Wo.ld, w_panel=Wo.panel, bias=bd.data_ptr() if bias else None,
                         residual=Ro.ptr if Ro else None, ldr=Ro.ld if Ro else 0, r_panel=Ro.panel if Ro else 0, out=Oo.ptr, ldo=Oo.ld,
                         o_panel=Oo.panel, out_f32=int(out_f32), pre_out=Po.ptr if Po else None, ldp=Po.ld if Po else 0,
                         p_panel=Po.panel if Po else 0, pre_kind=pre_kind or 0, act=act, act_grad=act_grad,
                         ln_gamma=gd.data_ptr() if ln else None, ln_beta=btd.data_ptr() if ln else None, ln_eps=1e-12,
                         drop=C.pointer(d) if d is not None else None, M=M, N=N, K=K)
    check(lib().mh_gemm_desc_launch(C.byref(desc), current_stream()), "mh_gemm_desc_launch")
    torch.cuda.synchronize()
    rtol = RTOL_F32 if out_f32 else RTOL_BF16
    # the epilogue in the kernel's order: v = acc + bias -> (second output) -> act -> dropout -> residual add / act-gradient multiply
    v, tol = act_ref(pre, act), eb + (ACT_ATOL if act else 0.0)
    if pre_kind == 0:
        close("pre", Po.read(), pre, eb, RTOL_BF16)
    elif pre_kind == 1:
        # gelu'(pre): the fast derivative's 1.1e-4 (+ 1e-3 where |pre| < 1e-2, as tests/test_round3_kernels_gpu.py states it), and the
        # accumulation error through gelu'' (|gelu''| <= 0.4)
        close("gelu'(pre)", Po.read(), gelu_grad(pre), 2e-4 + 1e-3 * (pre.abs() < 1e-2) + 0.4 * eb, RTOL_BF16)
    if d is not None and drop:
        keep = torch.from_numpy(gc.dense_keep(M, N, drop, d.seed, d.offset))
        v = torch.where(keep, v / (1 - drop), torch.zeros_like(v))
        tol = tol / (1 - drop)
    if act_grad:
        r = R.double()
        f = r if act_grad == DERIV else (gelu_grad(r) if act_grad == GELU else 1 - torch.tanh(r) ** 2)
        v, tol = v * f, tol * f.abs() + (ACT_ATOL * v.abs() if act_grad != DERIV else 0.0)
    elif R is not None:
        v = v + R.double()
    if ln:
        p_got = Po.read()
        close("pre-LayerNorm rows", p_got, v, tol, RTOL_BF16)
        # the training form normalises the rows it stores, rounded to bf16 (what a separate LayerNorm kernel reading them would see): the
        # LayerNorm is checked on those; what is left is its fp32 arithmetic (a few ulps of the normalised value)
        v = p_got.double()
        mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
        v = (v - mu) / torch.sqrt(var + 1e-12) * gamma.double() + beta.double()
        tol = 2.0 ** -16
    close("out", Oo.read(), v, tol, rtol)


# (variant name, census key, runner, kwargs, shape classes {class: (M, N, K, extra kwargs)})
WIDE_N = 512


def _std_multi(N):
    return multi_rows(256, -(-N // 128), 2)


def _shapes(panel_out, wide=False, rowpp=False):
    """the shape classes of a variant: ragged, multi-tile (and row window where the operands are panels)"""
    # (one block per CU on the 128 x 512 and 256 x 256 tiles: 2 slots + r tiles of 64 K 512 columns are 4.6 GFLOP of reference at K = 64,
    # 6.9 at K = 96 - the multi-tile shapes of these two tiles take K = 64, two K-steps of 32)
    if rowpp:       # the 128 x 512 full-row tile, one block per CU: N = 512 always
        return {"ragged": (1000, 512, 96), "multitile": (lambda: multi_rows(128, 1, 1), 512, 64), "window": (520, 512, 160)}
    if wide:        # the 256 x 256 tile is chosen for N % 256 == 0 when every CU gets a tile (device_cus()): ragged in M only
        return {"ragged": (lambda: (_cus() // 2 + 3) * 256 - 72, WIDE_N, 96),
                "multitile": (lambda: multi_rows(256, WIDE_N // 256, 1), WIDE_N, 64)}
    n = 288 if panel_out else 264
    s = {"ragged": (1000, n, 96), "multitile": (lambda: _std_multi(160 if panel_out else 136), 160 if panel_out else 136, 96)}
    if panel_out:
        s["window"] = (744, 160, 160)
    return s


VARIANTS = [
    # EPI 0, 256 x 128, fixed forms
    ("form1-rows", "gemm_big_kernel<C, 0, MH_ACT_NONE, (1 << 16)> | tile=256x128", run_dense, {}, _shapes(False)),
    ("form1-panels", "gemm_big_kernel<C, 0, MH_ACT_NONE, (1 << 16) | 16384> | tile=256x128", run_dense, dict(panels="awo"), _shapes(True)),
    ("form1-rows-wide", "gemm_big_kernel<C, 0, MH_ACT_NONE, (1 << 16)> | tile=256x256", run_dense, {}, _shapes(False, wide=True)),
    ("form2-rows", "gemm_big_kernel<C, 0, MH_ACT_NONE, (2 << 16)> | tile=256x128", run_dense, dict(res=True), _shapes(False)),
    ("form2-panels", "gemm_big_kernel<C, 0, MH_ACT_NONE, (2 << 16) | 16384> | tile=256x128", run_dense, dict(res=True, panels="awor"),
     _shapes(True)),
    ("form4-rows", "gemm_big_kernel<C, 0, MH_ACT_NONE, (4 << 16)> | tile=256x128", run_dense, dict(act_grad=DERIV, bias=False), _shapes(False)),
    ("form4-panels", "gemm_big_kernel<C, 0, MH_ACT_NONE, (4 << 16) | 16384> | tile=256x128", run_dense,
     dict(act_grad=DERIV, bias=False, panels="awor"), _shapes(True)),
    ("form8-rows", "gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, (8 << 16)> | tile=256x128", run_dense, dict(act=GELU, pre_kind=1), _shapes(False)),
    ("form8-panels", "gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, (8 << 16) | 16384> | tile=256x128", run_dense,
     dict(act=GELU, pre_kind=1, panels="awop"), _shapes(True)),
    # EPI 0, generic epilogue
    ("generic-f32out", "gemm_big_kernel<C, 0, MH_ACT_NONE, (0)> | tile=256x128", run_dense, dict(out_f32=True), _shapes(False)),
    ("generic-tanh-pre-wide", "gemm_big_kernel<C, 0, MH_ACT_TANH, (0)> | tile=256x256", run_dense, dict(act=TANH, pre_kind=0),
     _shapes(False, wide=True)),
    ("silu", "gemm_big_kernel<C, 0, MH_ACT_SILU> | tile=256x128", run_dense, dict(act=SILU), _shapes(False)),
    ("dropout-res-rows", "gemm_big_kernel<C, 0, MH_ACT_NONE, 64> | tile=256x128", run_dense, dict(res=True, drop=0.1), _shapes(False)),
    # the column-strip kernel (dense + bias + GELU of K32 panels, the sampler's FFN1): M % 256 == 0, N % 128 == 0, K = 512 only, so no
    # ragged shape reaches it.  Its grid is (2 CUs / bands) blocks per band, at most half the band's tiles: both shapes below give every
    # block a run of two tiles (8 m-tiles x 8 strips in one band; 16 x 4 in 8 bands of 2 m-tiles), the second one crossing a strip
    ("strip", "gemm_strip_kernel<16, MH_ACT_GELU_ERF> | tile=256x128", run_dense, dict(act=GELU, panels="awo"),
     {"multitile": (2048, 1024, 512), "multitile-bands": (4096, 512, 512), "window": (1024, 256, 512)}),
    # EPI 3: dropout + residual + LayerNorm over full rows (training), the pre-LayerNorm rows as second output
    ("ln-dropout", "gemm_big_kernel<C, 3, MH_ACT_NONE, (64) | 16384> | tile=128x512pp", run_dense, dict(ln=True, drop=0.1, panels="awor"),
     _shapes(True, rowpp=True)),
    ("ln-nodrop-train", "gemm_big_kernel<C, 3, MH_ACT_NONE, (64) | 16384> | tile=128x512pp", run_dense, dict(ln=True, drop=0.0, panels="awp"),
     {"ragged": (1000, 512, 96)}),
]


def _cases():
    out = []
    for name, key, fn, kw, shapes in VARIANTS:
        for cls, (M, N, K) in shapes.items():
            out.append(pytest.param(key, fn, kw, cls, M, N, K, id="%s-%s" % (name, cls)))
    return out


@pytest.mark.parametrize("key,fn,kw,cls,M,N,K", _cases())
def test_dense_variant_against_reference(key, fn, kw, cls, M, N, K):
    M = M() if callable(M) else M
    kw = dict(kw)
    if cls.startswith("window"):
        kw["window"] = True
    recs = gc.record(lambda: fn(M, N, K, **kw))
    keys = {k for k, _ in recs}
    assert key in keys, "the launch took %s, not the variant under test (%s)" % (sorted(keys), key)


# ------------------------------------------------------------------------------------- EPI 3: mh_gemm_bias_res_ln (sampler)
@pytest.mark.parametrize("cls,M,K", [("ragged", 1000, 96), ("multitile", None, 96), ("window", 520, 160)])
def test_res_ln_full_row_tile_against_reference(cls, M, K):
    """out = LayerNorm(A W^T + bias + residual) gamma + beta, K32 panels (the sampler's attention-output and FFN2 denses, d_model 512)"""
    N = 512
    M = M or multi_rows(128, 1, 1)
    window = cls == "window"
    A, W, z, eb = operands(M, N, K, 7)
    b, R = rnd(N, seed=8, scale=0.3), rnd(M, N, seed=9).bfloat16()
    gamma, beta = 1 + 0.2 * rnd(N, seed=10), 0.1 * rnd(N, seed=11)
    Ao, Wo, Ro = in_operand(A, True, window), in_operand(W, True, window), in_operand(R, True, window)
    Oo = out_operand(M, N, True, window)
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    recs = gc.record(lambda: check(lib().mh_gemm_bias_res_ln(Ao.ptr, Ao.ld, 1, Wo.ptr, Wo.ld, 1, bd.data_ptr(), Ro.ptr, Ro.ld, 1, gd.data_ptr(),
                                                             btd.data_ptr(), 1e-12, Oo.ptr, Oo.ld, 1, M, N, K, current_stream())))
    assert "gemm_big_kernel<C, 3, MH_ACT_NONE, (0) | 16384> | tile=128x512pp" in {k for k, _ in recs}
    v = z + b.double() + R.double()
    mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-12)
    close("out", Oo.read(), (v - mu) * rstd * gamma.double() + beta.double(),
          2 * eb.max(1, keepdim=True).values * rstd * gamma.double().abs() + 2.0 ** -16, RTOL_BF16)


# ------------------------------------------------------------------------------------------------------ mh_gemm_batched
@pytest.mark.parametrize("batch,M,N,K,out_f32", [(3, 300, 136, 96, 0), (4, 257, 264, 160, 1), (32, 128, 40, 128, 0)])
def test_gemm_batched_against_reference(batch, M, N, K, out_f32):
    """batch x (A_b W_b^T + bias) with every operand at a stride larger than its matrix (padding rows between batch entries), ragged M / N:
    the blockIdx.y offsets of A, W and the output (the op-per-node tape's attention products and split-K weight gradients)"""
    g = torch.Generator().manual_seed(batch * 1000 + M)
    lda, ldw, ldo = K + 16, K + 8, N + 8
    sA, sW, sO = (M + 3) * lda, (N + 5) * ldw, (M + 2) * ldo
    Abuf = (torch.randn(batch * sA, generator=g) * 0.7).bfloat16()
    Wbuf = (torch.randn(batch * sW, generator=g) / math.sqrt(K)).bfloat16()
    b = rnd(N, seed=5, scale=0.3)
    odt = torch.float32 if out_f32 else torch.bfloat16
    out = torch.full((batch * sO,), float("nan"), dtype=odt, device=DEV)
    Ad, Wd, bd = Abuf.to(DEV), Wbuf.to(DEV), b.to(DEV)
    recs = gc.record(lambda: check(lib().mh_gemm_batched(Ad.data_ptr(), lda, sA, Wd.data_ptr(), ldw, sW, bd.data_ptr(), out.data_ptr(), ldo, sO,
                                                         out_f32, batch, M, N, K, MH_BF16, current_stream())))
    form = "(0)" if out_f32 else "(1 << 16)"     # fp32 output: the generic epilogue; bf16: form 1 (batch > 1 never takes the wide tile)
    assert "gemm_big_kernel<C, 0, MH_ACT_NONE, %s> | tile=256x128" % form in {k for k, _ in recs}, sorted({k for k, _ in recs})
    o = out.cpu()
    for i in range(batch):
        A = Abuf[i * sA:i * sA + M * lda].view(M, lda)[:, :K]
        W = Wbuf[i * sW:i * sW + N * ldw].view(N, ldw)[:, :K]
        ref = A.double() @ W.double().T + b.double()
        got = o[i * sO:i * sO + M * ldo].view(M, ldo)
        close("batch %d" % i, got[:, :N], ref, acc_bound(A, W, K), RTOL_F32 if out_f32 else RTOL_BF16)
        assert bool(torch.isnan(got[:, N:].float()).all()) and bool(torch.isnan(o[i * sO + M * ldo:(i + 1) * sO].float()).all()), \
            "batch %d: written outside its rows / columns" % i


# ----------------------------------------------------------------------------------- fp32 128 x 128 kernel (parity mode)
@pytest.mark.parametrize("M,N,K,act", [(1000, 729, 144, NONE), (300, 200, 48, GELU)])
def test_f32_gemm_against_reference(M, N, K, act):
    """compute_dtype 'fp32': gemm_kernel<float, EPI 0> (grid = tiles, not persistent: ragged shapes only)"""
    A, W = rnd(M, K, seed=21, scale=0.7), rnd(N, K, seed=22, scale=1 / math.sqrt(K))
    b = rnd(N, seed=23, scale=0.3)
    out = torch.full((M, N), float("nan"), device=DEV)
    Ad, Wd, bd = A.to(DEV), W.to(DEV), b.to(DEV)
    recs = gc.record(lambda: check(lib().mh_gemm_bias_act(Ad.data_ptr(), K, Wd.data_ptr(), K, bd.data_ptr(), None, 0, out.data_ptr(), N, 1,
                                                          M, N, K, act, MH_F32, current_stream())))
    assert "gemm_kernel<float, EPI> | tile=128x128 epi=0 dtype=0" in {k for k, _ in recs}
    ref = act_ref(A.double() @ W.double().T + b.double(), act)
    close("out", out, ref, acc_bound(A, W, K) + (ACT_ATOL if act else 0), RTOL_F32)


# ---------------------------------------------------------------------------------------------- weight gradients (gemm_tn_kernel)
@pytest.mark.parametrize("K,M,N,panel,key", [
    (1056, 136, 128, 0, "gemm_tn_kernel<2> | tile=256x128"),
    (4128, 392, 512, 0, "gemm_tn_kernel<8, 4> | tile=256x256"),
    (2080, 544, 512, 1, "gemm_tn_kernel<8, 4, true> | tile=256x256"),
])
def test_weight_gradient_against_reference(K, M, N, panel, key):
    """dW [M, N] = A^T B over K tokens in split slices + the column sums of A (the bias gradient); M not a multiple of the 256-row tile,
    K an odd number of 32-token steps"""
    A = (rnd(K, M, seed=31, scale=0.5)).bfloat16()
    B = (rnd(K, N, seed=32, scale=0.5)).bfloat16()
    S = int(lib().mh_gemm_dw_splits(K, M, N))
    n = M * N + M
    part = torch.full((S, n), float("nan"), device=DEV)
    if panel:
        Ao, Bo = Operand(A, True, r0=0, extra=32), Operand(B, True, r0=0, extra=32)
        args = (Ao.ptr, Ao.ld, Bo.ptr, Bo.ld)
    else:
        Ad, Bd = A.to(DEV), B.to(DEV)
        args = (Ad.data_ptr(), M, Bd.data_ptr(), N)
    recs = gc.record(lambda: check(lib().mh_gemm_dw_bias_ex(args[0], args[1], args[2], args[3], panel, part.data_ptr(), S, K, M, N, 1,
                                                            current_stream())))
    assert key in {k for k, _ in recs}, sorted({k for k, _ in recs})
    got = part.double().sum(0).cpu()
    ref = A.double().T @ B.double()
    bound = K * 2.0 ** -24 * torch.outer(A.double().norm(dim=0), B.double().norm(dim=0))
    close("dW", got[:M * N].view(M, N), ref, bound, RTOL_F32)
    close("column sums", got[M * N:], A.double().sum(0), K * 2.0 ** -24 * A.double().abs().sum(0), RTOL_F32)


# ---------------------------------------------------------------------------------------------------- split precision
TDT = {MH_BF16X3: torch.bfloat16, MH_F16X3: torch.float16}
SPLIT_MODES = [pytest.param(MH_BF16X3, id="bf16x3"), pytest.param(MH_F16X3, id="f16x3")]


def split_pack(x, dt, ld=None):
    rows, cols = x.shape
    kpad = (cols + 31) // 32 * 32
    ld = ld or rows
    xd = x.to(DEV).float().contiguous()
    out = torch.zeros(2 * (kpad // 32) * ld * 32, dtype=TDT[dt], device=DEV)
    check(lib().mh_split_pack(xd.data_ptr(), cols, out.data_ptr(), ld, rows, cols, kpad, dt, current_stream()), "mh_split_pack")
    return out


@functools.lru_cache(maxsize=4)
def split_operands(M, N, K, seed):
    A, W = rnd(M, K, seed=seed, scale=0.7), rnd(N, K, seed=seed + 1, scale=1 / math.sqrt(K))
    return A, W, A.double() @ W.double().T


def _split_multi():
    return multi_rows(256, 2, 2)      # N = 136: two column tiles of 128, the second ragged


@pytest.mark.parametrize("dt", SPLIT_MODES)
@pytest.mark.parametrize("act,mode,res,cls", [(NONE, 1, False, "ragged"), (NONE, 1, True, "multitile"), (NONE, 2, False, "ragged"),
                                              (NONE, 2, False, "multitile"), (TANH, 0, False, "ragged"), (TANH, 0, False, "multitile"),
                                              (GELU, 0, False, "ragged"), (GELU, 0, True, "multitile")])
def test_split_gemm_against_reference(dt, act, mode, res, cls):
    """split_gemm_kernel (persistent, 2 blocks per CU, guard-free copy of the epilogue for interior tiles) in its three output forms"""
    M, N, K = (1000, 264 if mode == 2 else 288, 96) if cls == "ragged" else (_split_multi(), 136 if mode == 2 else 160, 96)
    A, W, z = split_operands(M, N, K, 41)
    b = rnd(N, seed=43, scale=0.3)
    R = rnd(M, N, seed=44) if res else None
    ref = act_ref(z + b.double(), act) + (R.double() if res else 0)
    Ap, Wp, bd = split_pack(A, dt), split_pack(W, dt), b.to(DEV)
    Rp = split_pack(R, dt) if res else None
    if mode == 2:
        out, ldo, part = torch.full((M, N), float("nan"), device=DEV), N, 0
    elif mode == 0:
        out, ldo, part = torch.full((2 * (N // 32) * M * 32,), float("nan"), dtype=TDT[dt], device=DEV), M, 0
    else:
        out, ldo, part = torch.full((2, M, N), float("nan"), dtype=TDT[dt], device=DEV), N, M * N
    recs = gc.record(lambda: check(lib().mh_split_gemm(Ap.data_ptr(), M, Wp.data_ptr(), N, bd.data_ptr(), 0, Rp.data_ptr() if res else None, M,
                                                       out.data_ptr(), ldo, mode, part, M, N, K, act, dt, current_stream()), "mh_split_gemm"))
    act_name = {NONE: "MH_ACT_NONE", TANH: "MH_ACT_TANH", GELU: "MH_ACT_GELU_ERF"}[act]
    assert "split_gemm_kernel<T, %s> | tile=256x128 out=%d" % (act_name, mode) in {k for k, _ in recs}
    if mode == 2:
        got = out.cpu().double()
    elif mode == 0:
        o = out.view(2, N // 32, M, 32).cpu().double()
        assert bool(torch.isfinite(o).all()), "unwritten elements"
        got = (o[0] + o[1]).permute(1, 0, 2).reshape(M, N)
    else:
        o = out.cpu().double()
        assert bool(torch.isfinite(o).all()), "unwritten elements"
        got = o[0] + o[1]
    tol = GEMM_TOL[dt]
    close("out", got, ref, tol * float(ref.pow(2).mean().sqrt()), tol)


@pytest.mark.parametrize("dt", SPLIT_MODES)
def test_split_gemm_res_ln_against_reference(dt):
    """split_gemm_ln_kernel (blocks own 128 complete rows; grid = row tiles, not persistent): ragged M, K an odd number of 32-steps"""
    M, N, K = 1000, 512, 96
    A, W, z = split_operands(M, N, K, 51)
    b, R = rnd(N, seed=53, scale=0.3), rnd(M, N, seed=54)
    gamma, beta = 1 + 0.2 * rnd(N, seed=55), 0.1 * rnd(N, seed=56)
    Ap, Wp, Rp = split_pack(A, dt), split_pack(W, dt), split_pack(R, dt)
    out = torch.full((2 * (N // 32) * M * 32,), float("nan"), dtype=TDT[dt], device=DEV)
    bd, gd, btd = b.to(DEV), gamma.to(DEV), beta.to(DEV)
    recs = gc.record(lambda: check(lib().mh_split_gemm_res_ln(Ap.data_ptr(), M, Wp.data_ptr(), N, bd.data_ptr(), Rp.data_ptr(), M, gd.data_ptr(),
                                                              btd.data_ptr(), 1e-12, out.data_ptr(), M, M, N, K, dt, current_stream())))
    assert "split_gemm_ln_kernel<T> | tile=128x512" in {k for k, _ in recs}
    v = z + b.double() + R.double()
    mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    ref = (v - mu) / torch.sqrt(var + 1e-12) * gamma.double() + beta.double()
    o = out.view(2, N // 32, M, 32).cpu().double()
    assert bool(torch.isfinite(o).all()), "unwritten elements"
    got = (o[0] + o[1]).permute(1, 0, 2).reshape(M, N)
    tol = GEMM_TOL[dt]
    close("out", got, ref, tol * float(ref.pow(2).mean().sqrt()), tol)


# ------------------------------------------------------------------------------------- deferred LayerNorm operands (EPI 0, 256 x 128)
def _row_stats(x, slots):
    """(sum, sum of squares) of each row of x in `slots` partial sums over column chunks: [rows, slots, 2] fp32, as a producer writes them"""
    parts = torch.chunk(x.double(), slots, dim=1)
    return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], -1) for p in parts], 1).float()


def _mean_rstd(st, h, eps):
    """the kernel's statistics from the partial sums (fp32 sums, var = E[x^2] - mean^2), in float64"""
    s = st.double().sum(1)
    mean = s[:, 0] / h
    var = (s[:, 1] / h - mean * mean).clamp_min(0)
    return mean[:, None], 1 / torch.sqrt(var + eps)[:, None]


DEFER_SHAPES = {"ragged": (1000, 288, 96), "multitile": (lambda: _std_multi(160), 160, 96), "window": (744, 160, 160)}


@pytest.mark.parametrize("cls", list(DEFER_SHAPES))
@pytest.mark.parametrize("form,key", [pytest.param(f, k, id=f) for f, k in (
    ("a-gelu", "gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, (128) | 16384> | tile=256x128"),
    ("r", "gemm_big_kernel<C, 0, MH_ACT_NONE, (256) | 16384> | tile=256x128"),
    ("o", "gemm_big_kernel<C, 0, MH_ACT_NONE, (512) | 16384> | tile=256x128"),
    ("r-o", "gemm_big_kernel<C, 0, MH_ACT_NONE, (768) | 16384> | tile=256x128"))])
def test_deferred_layernorm_variant_against_reference(form, key, cls):
    """mh_gemm_bias_act_defer (K32 panels): A rows raw (a: out = act(rstd_a (A W^T - mean_a c1) + c2)), residual rows raw (r: + (R - mean_r)
    rstd_r gamma + beta), output row statistics per 128-column tile (o: the sums of the bf16-rounded output values)"""
    M, N, K = DEFER_SHAPES[cls]
    M = M() if callable(M) else M
    window = cls == "window"
    da, dr, do = form.startswith("a"), "r" in form, "o" in form
    act = GELU if da else NONE
    g = torch.Generator().manual_seed(61)
    A = (torch.randn(M, K, generator=g) * 0.7 + 0.3).bfloat16()          # a non-zero mean: the mean_a c1 term matters
    W = (torch.randn(N, K, generator=g) * (1.5 / math.sqrt(K))).bfloat16()
    b, c1 = rnd(N, seed=62, scale=0.3), rnd(N, seed=63, scale=0.5)
    R = (torch.randn(M, N, generator=g) * 1.3 - 0.4).bfloat16() if dr else None
    rg, rb = 1 + 0.2 * rnd(N, seed=64), 0.1 * rnd(N, seed=65)
    eps, h = 1e-12, K if da else N
    a_st, r_st = _row_stats(A, 3) if da else None, _row_stats(R, 2) if dr else None
    o_slots = -(-N // 128) + 1                      # one slot more than the column tiles: it must stay untouched
    o_st = torch.full((M, o_slots, 2), float("nan"), device=DEV)
    dev = {k: v.to(DEV) for k, v in dict(b=b, c1=c1, rg=rg, rb=rb).items()}
    a_std, r_std = (a_st.to(DEV) if da else None), (r_st.to(DEV) if dr else None)
    d = _lib.LnDefer(a_stats=a_std.data_ptr() if da else None, a_slots=3 if da else 0, c1=dev["c1"].data_ptr() if da else None,
                     r_stats=r_std.data_ptr() if dr else None, r_slots=2 if dr else 0, r_gamma=dev["rg"].data_ptr() if dr else None,
                     r_beta=dev["rb"].data_ptr() if dr else None, o_stats=o_st.data_ptr() if do else None, o_slots=o_slots if do else 0,
                     h_norm=h, eps=eps)
    Ao, Wo = in_operand(A, True, window), in_operand(W, True, window)
    Ro = in_operand(R, True, window) if dr else None
    Oo = out_operand(M, N, True, window)
    recs = gc.record(lambda: check(lib().mh_gemm_bias_act_defer(Ao.ptr, Ao.ld, Wo.ptr, Wo.ld, dev["b"].data_ptr(), Ro.ptr if dr else None,
                                                                Ro.ld if dr else 0, Oo.ptr, Oo.ld, M, N, K, act, C.byref(d), current_stream()),
                                   "mh_gemm_bias_act_defer"))
    assert key in {k for k, _ in recs}, sorted({k for k, _ in recs})
    z = A.double() @ W.double().T
    tol = acc_bound(A, W, K)
    if da:
        mean, rstd = _mean_rstd(a_st, h, eps)
        mc = mean * c1.double()
        v = rstd * (z - mc) + b.double()
        # the accumulation error and the fp32 statistics (a few ulps of rstd and of mean c1) carried through rstd
        tol = rstd * (tol + 2.0 ** -20 * (z.abs() + mc.abs()))
        v, tol = act_ref(v, act), tol + ACT_ATOL
    else:
        v = z + b.double()
    if dr:
        mean, rstd = _mean_rstd(r_st, h, eps)
        v = v + (R.double() - mean) * rstd * rg.double() + rb.double()
        tol = tol + 2.0 ** -20 * ((R.double() - mean).abs() * rstd * rg.double().abs() + rb.double().abs())
    got = Oo.read()
    close("out", got, v, tol, RTOL_BF16)
    st = o_st.cpu().double()
    if do:
        # the statistics the consumer reads: sums over each column tile of the output as stored (bf16); 128 fp32 additions each
        y = got.double()
        for t in range(o_slots - 1):
            part = y[:, 128 * t:128 * (t + 1)]
            for j, ref in enumerate((part.sum(1), (part * part).sum(1))):
                mag = part.abs().sum(1) if j == 0 else (part * part).sum(1)
                close("o_stats[:, %d, %d]" % (t, j), st[:, t, j], ref, 128 * 2.0 ** -24 * mag + 1e-30, 0.0)
        assert bool(torch.isnan(st[:, -1]).all()), "o_stats written beyond the column tiles"
    else:
        assert bool(torch.isnan(st).all()), "o_stats written without a deferred output"


# ---------------------------------------------------------------------------------------------- QKV projection with the head scatter
def _vt_perm(vt):
    """[..., dh, L] -> keys of every group of 16 stored as 0-3, 8-11, 4-7, 12-15 (mh_gemm_qkv_vtperm's order)"""
    *lead, L = vt.shape
    return vt.reshape(*lead, L // 16, 4, 4)[..., [0, 2, 1, 3], :].reshape(*lead, L)


def _qkv_multi_batches(L, H):
    """batches B of seq_len L for a multi-tile launch of ceil(B L / 256) x ceil(3 H / 128) tiles"""
    M = multi_rows(256, -(-3 * H // 128), 2)
    return -(-M // L)


# (B, L, H, nh): ragged (B L % 256 != 0, 3 H % 128 != 0); multi-tile (B chosen from the CU count); row window
QKV_SHAPES = {"ragged": (3, 176, 320, 5), "multitile": (None, 512, 64, 2), "window": (2, 208, 128, 2)}


@pytest.mark.parametrize("cls", list(QKV_SHAPES))
@pytest.mark.parametrize("defer", [False, True], ids=["plain", "defer-a"])
def test_qkv_projection_against_reference(defer, cls):
    """mh_gemm_qkv_vtperm / _defer with K32-panel operands (the engine's launches: stage DMA as buffer loads): q, k [B, nh, L, dh] and
    V^T in the streaming attention's key order, every element against float64"""
    B, L, H, nh = QKV_SHAPES[cls]
    B = B or _qkv_multi_batches(L, H)
    M, N, K, dh = B * L, 3 * H, H, H // nh
    window = cls == "window"
    g = torch.Generator().manual_seed(71)
    A = (torch.randn(M, K, generator=g) * 0.7 + (0.3 if defer else 0.0)).bfloat16()
    W = (torch.randn(N, K, generator=g) * (1.5 / math.sqrt(K))).bfloat16()
    b, c1 = rnd(N, seed=72, scale=0.3), rnd(N, seed=73, scale=0.5)
    Ao, Wo = in_operand(A, True, window), in_operand(W, True, window)
    q = torch.full((B, nh, L, dh), float("nan"), device=DEV, dtype=torch.bfloat16)
    k = torch.full_like(q, float("nan"))
    vt = torch.full((B * H * L + 128,), float("nan"), device=DEV, dtype=torch.bfloat16)
    bd, c1d = b.to(DEV), c1.to(DEV)
    z = A.double() @ W.double().T
    tol = acc_bound(A, W, K)
    if defer:
        a_st = _row_stats(A, 2)
        a_std = a_st.to(DEV)
        d = _lib.LnDefer(a_stats=a_std.data_ptr(), a_slots=2, c1=c1d.data_ptr(), r_stats=None, r_slots=0, r_gamma=None, r_beta=None,
                         o_stats=None, o_slots=0, h_norm=K, eps=1e-12)
        run = lambda: check(lib().mh_gemm_qkv_vtperm_defer(Ao.ptr, Ao.ld, Wo.ptr, Wo.ld, bd.data_ptr(), q.data_ptr(), k.data_ptr(),  # noqa: E731
                                                           vt.data_ptr(), B, L, H, nh, C.byref(d), current_stream()), "qkv_vtperm_defer")
        key = "gemm_big_kernel<C, 1, MH_ACT_NONE, (128) | 16384> | tile=256x128"
        mean, rstd = _mean_rstd(a_st, K, 1e-12)
        mc = mean * c1.double()
        ref = rstd * (z - mc) + b.double()
        tol = rstd * (tol + 2.0 ** -20 * (z.abs() + mc.abs()))
    else:
        run = lambda: check(lib().mh_gemm_qkv_vtperm(Ao.ptr, Ao.ld, 1, Wo.ptr, Wo.ld, 1, bd.data_ptr(), q.data_ptr(), k.data_ptr(),  # noqa: E731
                                                     vt.data_ptr(), B, L, H, nh, current_stream()), "qkv_vtperm")
        key = "gemm_big_kernel<C, 1, MH_ACT_NONE, (32) | 16384> | tile=256x128"
        ref = z + b.double()
    recs = gc.record(run)
    assert key in {k_ for k_, _ in recs}, sorted({k_ for k_, _ in recs})
    heads = lambda x: x.reshape(B, L, nh, dh).permute(0, 2, 1, 3)  # noqa: E731
    close("q", q, heads(ref[:, :H]), heads(tol[:, :H]), RTOL_BF16)
    close("k", k, heads(ref[:, H:2 * H]), heads(tol[:, H:2 * H]), RTOL_BF16)
    vts = vt[:B * H * L].view(B, nh, dh, L)
    close("v^T (permuted keys)", vts, _vt_perm(heads(ref[:, 2 * H:]).transpose(-1, -2)), _vt_perm(heads(tol[:, 2 * H:]).transpose(-1, -2)),
          RTOL_BF16)
