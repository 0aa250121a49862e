"""The denoiser engine (csrc/engine.hip) restated for its tests (imported by test modules; not a conftest):

  plan(desc, B, L, knobs)          the path mh_denoiser_forward takes, as a key, from the library's public queries alone
  workspace_layout(desc, B, L)     the regions the engine carves out of its one workspace (offsets, sizes, aliasing)
  run_chain(eng, x, emb_t, ...)    the same C-ABI calls in the same order with the same arguments, but every activation, statistics and
                                   intermediate buffer a fresh allocation of its own, NaN-filled (0xFF bytes), never aliased, never in place
  time_chain(eng, t)               the same for mh_time_embed

The engine must equal the chain bit for bit: its kernels are deterministic, so the only thing that can differ is how the engine wires them
into shared memory.  CASES is the table of tests/test_engine_matrix_gpu.py; tests/test_engine_plan_cpu.py checks on the host that the
table reaches every path key."""
import collections
import contextlib
import ctypes as C
import math

import numpy as np

from musediffusion_amd import _lib
from musediffusion_amd._lib import ACT_GELU_ERF, ACT_NONE, ACT_SILU, ACT_TANH, MH_BF16, MH_BF16X3, MH_F16X3, MH_F32

DTYPE_NAME = {MH_F32: "f32", MH_BF16: "bf16", MH_BF16X3: "bf16x3", MH_F16X3: "f16x3"}
LOG2E_F32 = np.float32(1.4426950408889634)


def align256(v):
    return (v + 255) // 256 * 256


def pad64(v):
    return (v + 63) // 64 * 64


def esize(dtype):
    return 2 if dtype == MH_BF16 else 4       # (split precision: two 16-bit parts per element)


def is_split(dtype):
    return dtype in (MH_BF16X3, MH_F16X3)


# ------------------------------------------------------------------------------------------------------------------ workspace
Layout = collections.namedtuple("Layout", "regions forward time_embed total ffn_aliased")


def workspace_layout(desc, B, L, inplace=True, alias=True):
    """`carve` and mh_denoiser_workspace_bytes restated.  regions: name -> (offset, bytes asked for); every region starts on a 256-byte
    boundary.  inplace / alias follow the library's MH_WS_INPLACE / MH_WS_ALIAS build macros (both 1 in the product)."""
    N, es, H, F = B * L, esize(desc.dtype), desc.H, desc.F
    regions, off = collections.OrderedDict(), 0

    def take(name, nbytes):
        nonlocal off
        regions[name] = (off, nbytes)
        off += align256(nbytes)

    take("xin", N * desc.E_pad * es)
    take("buf1", N * H * es)
    take("bufX", N * H * es)
    if inplace:
        regions["bufX1"] = regions["bufX"]
    else:
        take("bufX1", N * H * es)
    qkv0 = off
    take("q", N * H * es)
    take("k", N * H * es)
    take("vt", N * H * es + 256)          # the slack behind V^T
    take("buf0", N * H * es)
    aliased = bool(alias and N * F * es <= off - qkv0)
    if aliased:
        regions["ffn"] = (qkv0, N * F * es)
    else:
        take("ffn", N * F * es)
    slots = (H + 127) // 128
    take("stats1", N * slots * 2 * 4)
    take("stats2", N * slots * 2 * 4)
    te = align256(B * desc.Tt_pad * 4) + align256(B * desc.T4_pad * 4)
    return Layout(regions, off, te, max(off, te), aliased)


def build_macros():
    """(inplace, alias) the loaded library was built with, read off the workspace size of a probe shape at which the four combinations
    differ: the product has both on; an A/B build with -DMH_WS_INPLACE=0 / -DMH_WS_ALIAS=0 must pass the same tests"""
    d, keep = dummy_desc(case("probe", 32, 128, 4, 256, 1, 1, 8, ""))
    got = _lib.lib().mh_denoiser_workspace_bytes(C.byref(d), 1, 8)
    hits = [(i, a) for i in (True, False) for a in (True, False) if workspace_layout(d, 1, 8, i, a).total == got]
    assert len(hits) == 1, (got, hits)
    return hits[0]


def time_layout(desc, B):
    """mh_time_embed's own two regions (sinusoid rows, hidden rows) and the bytes it asks for"""
    es = 4 if is_split(desc.dtype) else esize(desc.dtype)
    hid = align256(B * desc.Tt_pad * es)
    return hid, hid + align256(B * desc.T4_pad * es)


# ------------------------------------------------------------------------------------------------------------------ path key
def folded(desc):
    """the layer table carries the deferred-LayerNorm operands of every layer"""
    return all(desc.layers[l].w_ff1_f and (l == 0 or desc.layers[l].w_qkv_f) for l in range(desc.nL))


def plan(desc, B, L, knobs=None):
    """The path denoiser_run takes for this descriptor and shape under the library's current switch state.  knobs: what has no getter -
    prescale_q (the debug library's switch, default 0) and want ("out", "sqnorm" or "round": the entry point called)."""
    k = dict(prescale_q=0, want="out")
    k.update(knobs or {})
    lib = _lib.lib()
    H, dh = desc.H, desc.H // desc.nh
    if is_split(desc.dtype):
        return "split-%s | proj=%d ln=%s" % (DTYPE_NAME[desc.dtype], desc.has_proj, "fused" if lib.mh_split_gemm_res_ln_supported(H) else "kernel")
    if not desc.panel:
        return "rowmajor-%s | proj=%d" % (DTYPE_NAME[desc.dtype], desc.has_proj)
    if not desc.has_proj:
        head = "none"
    else:
        head = "fused" if lib.mh_up_proj_ln_fused_supported(desc.E, desc.E_pad, H) else "chain"
    fuse_ln = bool(lib.mh_denoiser_get_fuse_ln() and lib.mh_gemm_bias_res_ln_supported(H))
    stream = bool(lib.mh_attention_stream_enabled() and lib.mh_attention_stream_supported(L, dh) and H % 64 == 0)
    pre = bool(stream and k["prescale_q"] and lib.mh_attention_stream_prescaled_supported(L, dh))
    mode = lib.mh_denoiser_get_defer_ln()
    defer = bool((mode == 2 or (mode == 1 and not fuse_ln)) and stream and desc.nL > 0 and folded(desc))
    if desc.nL == 0:
        attn = ln = "none"
    else:
        attn = "stream-prescaled" if pre else ("stream" if stream else "tiled")
        ln = "defer" if defer else ("epilogue" if fuse_ln else "kernel")
    if not desc.has_proj:
        tail = "unpack"
    elif k["want"] == "round":
        tail = "round"
    else:
        tail = "fused" if lib.mh_down_proj_fused_supported(desc.E, H) else "chain"
    return "panel | head=%s attn=%s ln=%s tail=%s" % (head, attn, ln, tail)


# ------------------------------------------------------------------------------------------------------------------ the case table
def case(name, E, H, nh, F, nL, B, L, key, dtype=MH_BF16, panel=True, Tt=32, knobs=None, wants=("out",), V=97):
    return dict(name=name, E=E, H=H, nh=nh, F=F, nL=nL, B=B, L=L, key=key, dtype=dtype, panel=panel, Tt=Tt, knobs=dict(knobs or {}),
                wants=tuple(wants), V=V)


PANEL = "panel | head=%s attn=%s ln=%s tail=%s"
ALL_FUSED = (128, 512, 8, 1024, 2, 2, 512)
RAGGED = (64, 256, 4, 512, 2, 3, 528)
DEFER_768 = (128, 768, 12, 1536, 3, 1, 512)
TINY = (32, 64, 4, 256, 2, 2, 16)          # `tiny` and `same` of oracle/fixtures.py
SAME = (64, 64, 2, 128, 1, 3, 24)
CASES = [
    case("all-fused", *ALL_FUSED, PANEL % ("fused", "stream", "epilogue", "fused"), wants=("out", "sqnorm", "round", "round+upd"), V=729),
    case("ragged", *RAGGED, PANEL % ("fused", "stream", "epilogue", "fused"), wants=("out", "sqnorm")),
    case("chain-128", 32, 128, 4, 256, 2, 3, 40, PANEL % ("chain", "tiled", "epilogue", "chain")),
    case("wide-E", 132, 512, 8, 1024, 1, 2, 512, PANEL % ("chain", "stream", "epilogue", "chain")),
    case("defer-768", *DEFER_768, PANEL % ("fused", "stream", "defer", "fused"), wants=("out", "sqnorm")),
    case("kernel-768", 128, 768, 12, 1536, 2, 2, 64, PANEL % ("fused", "tiled", "kernel", "fused")),
    case("noproj-defer", 64, 64, 2, 128, 2, 2, 512, PANEL % ("none", "stream", "defer", "unpack")),
    case("big-F", 32, 128, 4, 1024, 1, 2, 40, PANEL % ("chain", "tiled", "epilogue", "chain")),
    case("no-layers", 128, 512, 8, 1024, 0, 2, 64, PANEL % ("fused", "none", "none", "fused")),
    case("rowmajor-f32-tiny", *TINY, "rowmajor-f32 | proj=1", dtype=MH_F32),
    case("rowmajor-f32-same", *SAME, "rowmajor-f32 | proj=0", dtype=MH_F32, Tt=16),
    case("rowmajor-bf16", 32, 128, 4, 256, 2, 3, 40, "rowmajor-bf16 | proj=1", panel=False),
    case("split-bf16x3", 32, 128, 4, 256, 2, 2, 40, "split-bf16x3 | proj=1 ln=kernel", dtype=MH_BF16X3),
    case("split-f16x3-same", *SAME, "split-f16x3 | proj=0 ln=kernel", dtype=MH_F16X3, Tt=16),
    case("split-bf16x3-512", 64, 512, 8, 1024, 1, 2, 40, "split-bf16x3 | proj=1 ln=fused", dtype=MH_BF16X3),
    # the debug library's switches (put back to the default after every test)
    case("all-fused/fuse_ln=0", *ALL_FUSED, PANEL % ("fused", "stream", "kernel", "fused"), knobs=dict(fuse_ln=0)),
    case("all-fused/defer_ln=2", *ALL_FUSED, PANEL % ("fused", "stream", "defer", "fused"), knobs=dict(defer_ln=2)),
    case("ragged/defer_ln=2", *RAGGED, PANEL % ("fused", "stream", "defer", "fused"), knobs=dict(defer_ln=2)),
    case("defer-768/defer_ln=0", *DEFER_768, PANEL % ("fused", "stream", "kernel", "fused"), knobs=dict(defer_ln=0)),
    case("all-fused/fuse_headtail=0", *ALL_FUSED, PANEL % ("chain", "stream", "epilogue", "chain"), knobs=dict(fuse_headtail=0)),
    case("all-fused/prescale_q=1", *ALL_FUSED, PANEL % ("fused", "stream-prescaled", "epilogue", "fused"), knobs=dict(prescale_q=1)),
    case("all-fused/defer_ln=2,prescale_q=1", *ALL_FUSED, PANEL % ("fused", "stream-prescaled", "defer", "fused"), knobs=dict(defer_ln=2, prescale_q=1)),
]
ROUND_KEY = PANEL % ("fused", "stream", "epilogue", "round")       # all-fused through mh_denoiser_forward_round
KNOB_DEFAULTS = dict(fuse_ln=1, defer_ln=1, fuse_headtail=1, prescale_q=0)
L_EXTRA = 16                # rows of the position table beyond L: the "residue of another shape" forward runs at L + 8


@contextlib.contextmanager
def switches(knobs):
    """the debug library with the case's switches on for the block; the defaults and the previous library are back after it.  No knobs:
    whichever library is current."""
    if not knobs:
        yield _lib.lib()
        return
    with _lib.debug_library() as lib:
        try:
            for name, v in knobs.items():
                _lib.check(getattr(lib, "mh_denoiser_set_" + name)(v), name)
            yield lib
        finally:
            for name in knobs:
                getattr(lib, "mh_denoiser_set_" + name)(KNOB_DEFAULTS[name])


def engine_cfg(c):
    return dict(E=c["E"], H=c["H"], F=c["F"], nh=c["nh"], nL=c["nL"], Tt=c["Tt"], L_max=c["L"] + L_EXTRA)


def dummy_desc(c):
    """The descriptor DenoiserEngine builds for a case (musediffusion_amd/engine.py: padded sizes, the panel rule, where the folded
    operands are packed), with dummy pointers: for the argument checks and the plan on a machine without a device.  Call it inside
    switches(c["knobs"]): defer_ln = 2 at construction packs the folded operands.  Returns (descriptor, keep-alive)."""
    lib = _lib.lib()
    d = _lib.Denoiser()
    dt, dh = c["dtype"], c["H"] // c["nh"]
    d.dtype = dt
    for k in ("E", "H", "F", "nh", "nL", "Tt"):
        setattr(d, k, c[k])
    d.E_pad, d.Tt_pad, d.T4_pad, d.L_max = pad64(c["E"]), pad64(c["Tt"]), pad64(4 * c["Tt"]), c["L"] + L_EXTRA
    d.has_proj = int(c["E"] != c["H"])
    d.panel = int(dt == MH_BF16 and c["panel"] and c["E"] % 4 == 0 and dh % 32 == 0 and c["H"] // 32 in (2, 4, 8, 12, 16, 24))
    d.ln_eps = 1e-12
    fold = bool(d.panel and (not lib.mh_gemm_bias_res_ln_supported(c["H"]) or lib.mh_denoiser_get_defer_ln() == 2))
    dummy = 0x1000
    for k in ("w_t0", "b_t0", "w_t2", "b_t2", "pos", "ln0_g", "ln0_b"):
        setattr(d, k, dummy)
    if d.has_proj:
        for k in ("w_up0", "b_up0", "w_up2", "b_up2", "w_dn0", "b_dn0", "w_dn2", "b_dn2"):
            setattr(d, k, dummy)
    layers = (_lib.LayerWeights * max(1, c["nL"]))()
    for l in range(c["nL"]):
        for k, _ in _lib.LayerWeights._fields_:
            is_f = k in ("w_qkv_f", "c1_qkv", "c2_qkv", "w_ff1_f", "c1_ff1", "c2_ff1")
            if not is_f or (fold and (l > 0 or "qkv" not in k)):
                setattr(layers[l], k, dummy)
    d.layers = C.cast(layers, C.POINTER(_lib.LayerWeights))
    return d, layers


# ------------------------------------------------------------------------------------------------------------------ the chain
class Fresh:
    """fresh device buffers, every byte 0xFF before use (NaN in fp32, bf16, f16 and both parts of a split value; -1 in int32), each with
    its own slack behind it.  `bufs` keeps them by role for the caller to read."""

    def __init__(self, slack=512):
        self.bufs = collections.OrderedDict()
        self.slack = slack

    def new(self, name, nbytes):
        import torch
        assert name not in self.bufs, name
        t = torch.full((int(nbytes) + self.slack,), 0xFF, dtype=torch.uint8, device="cuda")
        self.bufs[name] = t
        return t.data_ptr()


def softmax_scale(dh):
    """1.0f / sqrtf((float) dh) and that times log2(e), both in fp32 as the engine computes them"""
    scale = np.float32(1.0) / np.sqrt(np.float32(dh))
    return float(scale), float(np.float32(scale * LOG2E_F32))


def _defer(H, eps, **fields):
    d = _lib.LnDefer()
    d.h_norm, d.eps = H, eps
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def run_chain(eng, x, emb_t, emb_row, B, L, want="out", knobs=None, round_to=None, phases=None):
    """The launches of denoiser_run for `eng` on x [B, L, E] fp32 (device), in its order, over fresh unaliased buffers.
    want: "out" (mh_denoiser_forward), "sqnorm" (+ |row|^2), "round" (+ nearest table row; round_to = (table_split pointer, V, upd or None)).
    phases: None = the whole forward, or dict(mask=1 | 2 | 4, xh / xi / xo / xt=(pointer, ld)) as the phased entry points pass them.
    Returns dict(out, sqnorm, idx: host arrays or None; bufs: every buffer by role; key: plan())."""
    import torch
    lib, d, st = _lib.lib(), eng._desc, _lib.current_stream()
    k = dict(prescale_q=0, want="round" if want == "round" else "out")
    k.update(knobs or {})
    key = plan(d, B, L, k)
    N, H, F, E, E_pad, nh, nL, dt = B * L, d.H, d.F, d.E, d.E_pad, d.nh, d.nL, d.dtype
    dh, es, eps = H // nh, esize(dt), float(d.ln_eps)
    scale, q_scale = softmax_scale(dh)
    A = Fresh()
    W = eng._addr
    ph = dict(mask=7, xh=None, xi=None, xo=None, xt=None)
    ph.update(phases or {})
    mask = ph["mask"]
    xp, tp, rp = _lib.ptr(x), _lib.ptr(emb_t), _lib.ptr(emb_row)
    out = A.new("out", N * E * 4) if mask & 4 else None
    sq = A.new("sqnorm", N * 4) if want in ("sqnorm",) else None
    idx = A.new("idx", N * 4) if want == "round" else None

    def call(name, *args):
        _lib.check(getattr(lib, name)(*args, st), name)

    def LW(l, name):
        return W("l%d.%s" % (l, name))

    if d.panel:
        P = 1

        def gemm(a, lda, w, w_rows, bias, res, ldr, o, of32, ldo, Nout, K, act):
            call("mh_gemm_bias_act_ex", a, lda, P, w, w_rows, P, bias, res, ldr, P, o, ldo, 0 if of32 else P, of32, N, Nout, K, act, dt)

        def gemm_ln(a, w, bias, res, ldr, gamma, beta, o, ldo, K):
            call("mh_gemm_bias_res_ln", a, N, P, w, H, P, bias, res, ldr, P, gamma, beta, eps, o, ldo, P, N, H, K)

        rows = lambda name: (A.new(name, N * H * es), N)          # a K32-panel activation buffer of the chain's own
        head, attn, ln, tail = (f.split("=")[1] for f in key.split(" | ")[1].split())
        pre_q = attn == "stream-prescaled"
        XH = XI = XO = XT = None
        if mask & 1:
            XH = ph["xh"] or rows("x0")
            if head == "fused":
                call("mh_up_proj_ln_fused", xp, E, E_pad, W("w_up0"), W("b_up0"), W("w_up2"), W("b_up2"), W("pos"), tp, rp, W("ln0_g"), W("ln0_b"),
                     eps, XH[0], XH[1], B, L, H)
            elif head == "chain":
                xin = A.new("xin", N * E_pad * es)
                up0, up2 = A.new("up0", N * H * es), A.new("up2", N * H * es)
                call("mh_pack_panel", xp, E, xin, N, N, E, E_pad)
                gemm(xin, N, W("w_up0"), H, W("b_up0"), None, 0, up0, 0, N, H, E_pad, ACT_TANH)
                gemm(up0, N, W("w_up2"), H, W("b_up2"), None, 0, up2, 0, N, H, H, ACT_NONE)
                call("mh_add_pos_time_layernorm_panel", up2, N, 0, W("pos"), tp, rp, W("ln0_g"), W("ln0_b"), XH[0], XH[1], B, L, H, eps)
            else:
                call("mh_add_pos_time_layernorm_panel", xp, H, 1, W("pos"), tp, rp, W("ln0_g"), W("ln0_b"), XH[0], XH[1], B, L, H, eps)
        if mask & 2:
            XI = ph["xi"] or XH
            XO = ph["xo"] or (rows("xL") if nL else XI)
            S = (H + 127) // 128
            cur = XI                                             # this layer's input rows
            prev_stats = None                                    # deferred: `cur` holds raw rows with these statistics
            for l in range(nL):
                p = "l%d." % l
                last = l == nL - 1
                q, kk, vt, ctx = (A.new(p + n, N * H * es + (256 if n == "vt" else 0)) for n in ("q", "k", "vt", "ctx"))
                if ln == "defer":
                    if prev_stats is not None:
                        dd = _defer(H, eps, a_stats=prev_stats, a_slots=S, c1=LW(l, "c1_qkv"))
                        if pre_q:
                            call("mh_gemm_qkv_vtperm_qs", cur[0], cur[1], LW(l, "w_qkv_f"), 3 * H, LW(l, "c2_qkv"), q, kk, vt, B, L, H, nh, q_scale, C.byref(dd))
                        else:
                            call("mh_gemm_qkv_vtperm_defer", cur[0], cur[1], LW(l, "w_qkv_f"), 3 * H, LW(l, "c2_qkv"), q, kk, vt, B, L, H, nh, C.byref(dd))
                    elif pre_q:
                        call("mh_gemm_qkv_vtperm_qs", cur[0], cur[1], LW(l, "w_qkv"), 3 * H, LW(l, "b_qkv"), q, kk, vt, B, L, H, nh, q_scale, None)
                    else:
                        call("mh_gemm_qkv_vtperm", cur[0], cur[1], P, LW(l, "w_qkv"), 3 * H, P, LW(l, "b_qkv"), q, kk, vt, B, L, H, nh)
                elif attn != "tiled":
                    if pre_q:
                        call("mh_gemm_qkv_vtperm_qs", cur[0], cur[1], LW(l, "w_qkv"), 3 * H, LW(l, "b_qkv"), q, kk, vt, B, L, H, nh, q_scale, None)
                    else:
                        call("mh_gemm_qkv_vtperm", cur[0], cur[1], P, LW(l, "w_qkv"), 3 * H, P, LW(l, "b_qkv"), q, kk, vt, B, L, H, nh)
                else:
                    call("mh_gemm_qkv_ex", cur[0], cur[1], P, LW(l, "w_qkv"), 3 * H, P, LW(l, "b_qkv"), q, kk, vt, B, L, H, nh, dt)
                if attn == "tiled":
                    call("mh_attention_fwd_ex", q, kk, vt, ctx, N, P, B, L, nh, dh, scale, dt)
                elif pre_q:
                    call("mh_attention_stream_fwd_prescaled", q, kk, vt, ctx, N, P, B, L, nh, dh)
                else:
                    call("mh_attention_stream_fwd", q, kk, vt, ctx, N, P, B, L, nh, dh, scale)
                ffn = A.new(p + "ffn", N * F * es)
                if ln == "defer":
                    y1, s1 = A.new(p + "y1", N * H * es), A.new(p + "stats1", N * S * 8)
                    dd = _defer(H, eps, o_stats=s1, o_slots=S)
                    if prev_stats is not None:
                        dd.r_stats, dd.r_slots, dd.r_gamma, dd.r_beta = prev_stats, S, LW(l - 1, "ln2_g"), LW(l - 1, "ln2_b")
                    call("mh_gemm_bias_act_defer", ctx, N, LW(l, "w_ao"), H, LW(l, "b_ao"), cur[0], cur[1], y1, N, N, H, H, ACT_NONE, C.byref(dd))
                    dd = _defer(H, eps, a_stats=s1, a_slots=S, c1=LW(l, "c1_ff1"))
                    call("mh_gemm_bias_act_defer", y1, N, LW(l, "w_ff1_f"), F, LW(l, "c2_ff1"), None, 0, ffn, N, N, F, H, ACT_GELU_ERF, C.byref(dd))
                    y2 = A.new(p + "y2", N * H * es)
                    dd = _defer(H, eps, r_stats=s1, r_slots=S, r_gamma=LW(l, "ln1_g"), r_beta=LW(l, "ln1_b"))
                    if not last:
                        prev_stats = A.new(p + "stats2", N * S * 8)
                        dd.o_stats, dd.o_slots = prev_stats, S
                    call("mh_gemm_bias_act_defer", ffn, N, LW(l, "w_ff2"), H, LW(l, "b_ff2"), y1, N, y2, N, N, H, F, ACT_NONE, C.byref(dd))
                    if last:
                        call("mh_layernorm_panel", y2, N, LW(l, "ln2_g"), LW(l, "ln2_b"), XO[0], XO[1], N, H, eps)
                    cur = (y2, N)
                    continue
                x1 = rows(p + "x1")
                nxt = XO if last else rows(p + "x2")
                if ln == "epilogue":
                    gemm_ln(ctx, LW(l, "w_ao"), LW(l, "b_ao"), cur[0], cur[1], LW(l, "ln1_g"), LW(l, "ln1_b"), x1[0], N, H)
                else:
                    y1 = A.new(p + "y1", N * H * es)
                    gemm(ctx, N, LW(l, "w_ao"), H, LW(l, "b_ao"), cur[0], cur[1], y1, 0, N, H, H, ACT_NONE)
                    call("mh_layernorm_panel", y1, N, LW(l, "ln1_g"), LW(l, "ln1_b"), x1[0], N, N, H, eps)
                gemm(x1[0], N, LW(l, "w_ff1"), F, LW(l, "b_ff1"), None, 0, ffn, 0, N, F, H, ACT_GELU_ERF)
                if ln == "epilogue":
                    gemm_ln(ffn, LW(l, "w_ff2"), LW(l, "b_ff2"), x1[0], N, LW(l, "ln2_g"), LW(l, "ln2_b"), nxt[0], nxt[1], F)
                else:
                    y2 = A.new(p + "y2", N * H * es)
                    gemm(ffn, N, LW(l, "w_ff2"), H, LW(l, "b_ff2"), x1[0], N, y2, 0, N, H, F, ACT_NONE)
                    call("mh_layernorm_panel", y2, N, LW(l, "ln2_g"), LW(l, "ln2_b"), nxt[0], nxt[1], N, H, eps)
                cur = nxt
        if mask & 4:
            XT = ph["xt"] or XO
            if tail == "round":
                tsplit, V, upd = round_to
                call("mh_down_proj_round_fused", XT[0], XT[1], W("w_dn0"), W("b_dn0"), W("w_dn2"), W("b_dn2"), out, sq, tsplit, V, idx,
                     C.byref(upd) if upd is not None else None, N, E, H)
            elif tail == "fused":
                call("mh_down_proj_fused", XT[0], XT[1], W("w_dn0"), W("b_dn0"), W("w_dn2"), W("b_dn2"), out, sq, N, E, H)
            elif tail == "chain":
                dn0 = A.new("dn0", N * H * es)
                gemm(XT[0], XT[1], W("w_dn0"), H, W("b_dn0"), None, 0, dn0, 0, N, H, H, ACT_TANH)
                gemm(dn0, N, W("w_dn2"), E, W("b_dn2"), None, 0, out, 1, E, E, H, ACT_NONE)
            else:
                call("mh_unpack_panel_f32", XT[0], XT[1], out, E, N, E)
    elif is_split(dt):
        part_qk, part_vt = N * 2 * H, H * N
        fuse = key.endswith("ln=fused")

        def sgemm(a, w, w_rows, bias, res, o, ldo, mode, M2, Nout, K, act):
            call("mh_split_gemm", a, N, w, w_rows, bias, 0, res, N, o, ldo, mode, 0, M2, Nout, K, act, dt)

        cur = A.new("x0", N * H * 4)
        if d.has_proj:
            xin, up0, up2 = A.new("xin", N * E_pad * 4), A.new("up0", N * H * 4), A.new("up2", N * H * 4)
            call("mh_split_pack", xp, E, xin, N, N, E, E_pad, dt)
            sgemm(xin, W("w_up0"), H, W("b_up0"), None, up0, N, 0, N, H, E_pad, ACT_TANH)
            sgemm(up0, W("w_up2"), H, W("b_up2"), None, up2, H, 2, N, H, H, ACT_NONE)
            call("mh_split_layernorm", up2, H, W("pos"), tp, rp, W("ln0_g"), W("ln0_b"), cur, N, N, L, H, eps, dt)
        else:
            call("mh_split_layernorm", xp, H, W("pos"), tp, rp, W("ln0_g"), W("ln0_b"), cur, N, N, L, H, eps, dt)
        for l in range(nL):
            p = "l%d." % l
            qk, vt, ctx = A.new(p + "qk", N * 2 * H * 4), A.new(p + "vt", N * H * 4 + 256), A.new(p + "ctx", N * H * 4)
            x1, ffn, x2 = A.new(p + "x1", N * H * 4), A.new(p + "ffn", N * F * 4), A.new(p + "x2", N * H * 4)
            call("mh_split_gemm", cur, N, LW(l, "w_qkv"), 3 * H, LW(l, "b_qkv"), 0, None, 0, qk, 2 * H, 1, part_qk, N, 2 * H, H, ACT_NONE, dt)
            call("mh_split_gemm", LW(l, "w_qkv") + 2 * H * 32 * 2, 3 * H, cur, N, LW(l, "b_qkv") + 2 * H * 4, 1, None, 0, vt, N, 1, part_vt, H, N, H, ACT_NONE, dt)
            call("mh_split_attention", qk, 2 * H, H, part_qk, vt, N, part_vt, ctx, N, B, L, nh, dh, scale, dt)
            if fuse:
                call("mh_split_gemm_res_ln", ctx, N, LW(l, "w_ao"), H, LW(l, "b_ao"), cur, N, LW(l, "ln1_g"), LW(l, "ln1_b"), eps, x1, N, N, H, H, dt)
            else:
                y1 = A.new(p + "y1", N * H * 4)
                sgemm(ctx, LW(l, "w_ao"), H, LW(l, "b_ao"), cur, y1, H, 2, N, H, H, ACT_NONE)
                call("mh_split_layernorm", y1, H, None, None, None, LW(l, "ln1_g"), LW(l, "ln1_b"), x1, N, N, L, H, eps, dt)
            sgemm(x1, LW(l, "w_ff1"), F, LW(l, "b_ff1"), None, ffn, N, 0, N, F, H, ACT_GELU_ERF)
            if fuse:
                call("mh_split_gemm_res_ln", ffn, N, LW(l, "w_ff2"), H, LW(l, "b_ff2"), x1, N, LW(l, "ln2_g"), LW(l, "ln2_b"), eps, x2, N, N, H, F, dt)
            else:
                y2 = A.new(p + "y2", N * H * 4)
                sgemm(ffn, LW(l, "w_ff2"), H, LW(l, "b_ff2"), x1, y2, H, 2, N, H, F, ACT_NONE)
                call("mh_split_layernorm", y2, H, None, None, None, LW(l, "ln2_g"), LW(l, "ln2_b"), x2, N, N, L, H, eps, dt)
            cur = x2
        if d.has_proj:
            dn0 = A.new("dn0", N * H * 4)
            sgemm(cur, W("w_dn0"), H, W("b_dn0"), None, dn0, N, 0, N, H, H, ACT_TANH)
            sgemm(dn0, W("w_dn2"), E, W("b_dn2"), None, out, E, 2, N, E, H, ACT_NONE)
        else:
            call("mh_split_join", cur, N, out, E, N, E, H, dt)
    else:
        def gemm(a, lda, w, ldw, bias, res, ldr, o, ldo, of32, Nout, K, act):
            call("mh_gemm_bias_act", a, lda, w, ldw, bias, res, ldr, o, ldo, of32, N, Nout, K, act, dt)

        cur = A.new("x0", N * H * es)
        if d.has_proj:
            xin, up0, up2 = A.new("xin", N * E_pad * es), A.new("up0", N * H * es), A.new("up2", N * H * es)
            call("mh_cast_pad", xp, E, xin, E_pad, N, E, N, dt)
            gemm(xin, E_pad, W("w_up0"), E_pad, W("b_up0"), None, 0, up0, H, 0, H, E_pad, ACT_TANH)
            gemm(up0, H, W("w_up2"), H, W("b_up2"), None, 0, up2, H, 0, H, H, ACT_NONE)
            call("mh_add_pos_time_layernorm", up2, H, 0, W("pos"), tp, rp, W("ln0_g"), W("ln0_b"), cur, B, L, H, eps, dt)
        else:
            call("mh_add_pos_time_layernorm", xp, H, 1, W("pos"), tp, rp, W("ln0_g"), W("ln0_b"), cur, B, L, H, eps, dt)
        for l in range(nL):
            p = "l%d." % l
            q, kk, vt, ctx = (A.new(p + n, N * H * es + (256 if n == "vt" else 0)) for n in ("q", "k", "vt", "ctx"))
            y1, x1, ffn, y2, x2 = (A.new(p + n, N * (F if n == "ffn" else H) * es) for n in ("y1", "x1", "ffn", "y2", "x2"))
            call("mh_gemm_qkv", cur, H, LW(l, "w_qkv"), H, LW(l, "b_qkv"), q, kk, vt, B, L, H, nh, dt)
            call("mh_attention_fwd", q, kk, vt, ctx, H, B, L, nh, dh, scale, dt)
            gemm(ctx, H, LW(l, "w_ao"), H, LW(l, "b_ao"), cur, H, y1, H, 0, H, H, ACT_NONE)
            call("mh_layernorm", y1, LW(l, "ln1_g"), LW(l, "ln1_b"), x1, N, H, eps, dt)
            gemm(x1, H, LW(l, "w_ff1"), H, LW(l, "b_ff1"), None, 0, ffn, F, 0, F, H, ACT_GELU_ERF)
            gemm(ffn, F, LW(l, "w_ff2"), F, LW(l, "b_ff2"), x1, H, y2, H, 0, H, F, ACT_NONE)
            call("mh_layernorm", y2, LW(l, "ln2_g"), LW(l, "ln2_b"), x2, N, H, eps, dt)
            cur = x2
        if d.has_proj:
            dn0 = A.new("dn0", N * H * es)
            gemm(cur, H, W("w_dn0"), H, W("b_dn0"), None, 0, dn0, H, 0, H, H, ACT_TANH)
            gemm(dn0, H, W("w_dn2"), H, W("b_dn2"), None, 0, out, E, 1, E, H, ACT_NONE)
        else:
            call("mh_cast_to_f32", cur, H, out, E, N, E, dt)
    torch.cuda.synchronize()

    def host(name, n, dtype):
        if name not in A.bufs:
            return None
        t = A.bufs[name]
        assert bool((t[n * 4:] == 0xFF).all()), "the chain wrote behind its own %s" % name
        return t[:n * 4].view(dtype).cpu().numpy()

    res = dict(key=key, bufs=A.bufs, out=host("out", N * E, torch.float32), sqnorm=host("sqnorm", N, torch.float32), idx=host("idx", N, torch.int32))
    if res["out"] is not None:
        res["out"] = res["out"].reshape(B, L, E)
    return res


def time_chain(eng, t):
    """mh_time_embed as its three launches over buffers of its own: the sinusoid rows NaN-filled, the hidden rows zeroed (their padded
    columns are read as K of the second dense layer and written by nobody).  t [B] fp32 on the device -> [B, H] fp32 host array."""
    import torch
    lib, d, st = _lib.lib(), eng._desc, _lib.current_stream()
    B = t.numel()
    tdt = MH_F32 if is_split(d.dtype) else d.dtype
    es = esize(tdt)
    A = Fresh()
    sin, out = A.new("sin", B * d.Tt_pad * es), A.new("out", B * d.H * 4)
    hid = torch.zeros(B * d.T4_pad * es, dtype=torch.uint8, device="cuda")
    _lib.check(lib.mh_timestep_embedding(_lib.ptr(t), sin, B, d.Tt, d.Tt_pad, 10000.0, tdt, st), "mh_timestep_embedding")
    _lib.check(lib.mh_gemm_bias_act(sin, d.Tt_pad, eng._addr("w_t0"), d.Tt_pad, eng._addr("b_t0"), None, 0, hid.data_ptr(), d.T4_pad, 0, B, 4 * d.Tt,
                                    d.Tt_pad, ACT_SILU, tdt, st), "mh_gemm_bias_act")
    _lib.check(lib.mh_gemm_bias_act(hid.data_ptr(), d.T4_pad, eng._addr("w_t2"), d.T4_pad, eng._addr("b_t2"), None, 0, out, d.H, 1, B, d.H, d.T4_pad,
                                    ACT_NONE, tdt, st), "mh_gemm_bias_act")
    torch.cuda.synchronize()
    buf = A.bufs["out"]
    assert bool((buf[B * d.H * 4:] == 0xFF).all())
    return buf[:B * d.H * 4].view(torch.float32).cpu().numpy().reshape(B, d.H)


# ------------------------------------------------------------------------------------------------------------------ float64 reference
def timestep_embedding64(t, dim, max_period=10000):
    """oracle.denoiser.timestep_embedding in float64"""
    import torch
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float64) / half)
    args = t.double()[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def time_embed64(sd, t, Tt):
    import torch.nn.functional as F
    from oracle import denoiser as odn
    sd = {k: v.double() for k, v in sd.items() if k.startswith("time_embed")}
    return odn._lin(F.silu(odn._lin(timestep_embedding64(t, Tt), sd, "time_embed.0")), sd, "time_embed.2")


def forward64(sd, x, t, nh, Tt):
    """oracle.denoiser.forward evaluated in float64: state dict and inputs cast to double, the oracle's own layer function"""
    import torch.nn.functional as F
    from oracle import denoiser as odn
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.double()
    emb_t = time_embed64(sd, t, Tt)
    emb_x = odn._lin(F.tanh(odn._lin(x, sd, "input_up_proj.0")), sd, "input_up_proj.2") if "input_up_proj.0.weight" in sd else x
    h = sd["position_embeddings.weight"][:x.shape[1]][None] + emb_x + emb_t[:, None, :]
    h = F.layer_norm(h, (h.shape[-1],), sd["LayerNorm.weight"], sd["LayerNorm.bias"], 1e-12)
    for i in range(odn.count_layers(sd)):
        h = odn.encoder_layer(h, sd, i, nh)
    if "output_down_proj.0.weight" in sd:
        h = odn._lin(F.tanh(odn._lin(h, sd, "output_down_proj.0")), sd, "output_down_proj.2")
    return h
