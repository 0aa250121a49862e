"""Parity matrix of the streaming attention family: every instantiation the dispatchers can pick in the product build (csrc/attention_stream.hip:
kStreamProduct, 15 forward builds; csrc/attention_bwd.hip: launch_bwd, 8 <DH, DROP, FULL> pairs of kernels) against a float64 reference
on the CPU (tests/attention_ref.py), EVERY element of EVERY output, at the shapes where a persistent streaming kernel goes wrong:

* ragged (key-bound builds): seq_len 528 / 784 / 2096 - not a multiple of 256 nor of 32 (a 16-row last tile), a last query block in which
  most waves are idle, several stages with a partial last one; 3 x 5 (batch, head)s, so the grid is no multiple of 8 (mh_xcd_remap's
  remainder branch);
* multi-item: the kernels launch min(items, slots) blocks (slots = CUs; 2 CUs for the 8-wave dropout generator) and every block walks a
  flattened (item, stage) sequence, the next item's first K / V stage arriving under the current item's last tiles.  items = 2 slots + r
  (0 < r < slots), asserted from the recorded launch (2 grid < items < 3 grid); the number of heads is 3, 5 or 6 (bh / nh, bh % nh
  addressing across the walk), and a dominant key sits in the first stage of items a block reaches second and third.  seq_len 512 for
  most of them (the float64 reference is the cost), 1024 for the FULL builds as the training step launches them;
* layouts: q / k / v as [B, nh, L, dh] tensors and as column blocks of the token-major [B L, 3 H] projection; the context rows (and dQ | dK |
  dV) row-major with a padded pitch and as K32 panels that are a row window of a larger buffer.

Each case records its launch (tests/attention_census.py) and asserts which variant it ran.  Every output buffer starts as NaN (keep bits: a
sentinel behind the tensor): afterwards everything inside is finite and everything outside - pad columns, window rows, the slack behind
lse2 / D - is untouched.  Backward cases are isolated from the forward kernel: they read O (bf16) and lse2 (fp32) of the REFERENCE, so a
forward error can neither cause nor mask a backward failure; one case per head dim chains forward -> backward as training does.
Dropout: the reference mask is decoded from the bit tensor (tests/test_dropout_gpu.py: bits_to_mask) - the one the generator wrote, which
must equal mh_dropout_bits word for word, or random words the test wrote for the bit reader.

Tolerances are per element, |got - ref| <= atol_i + rtol |ref_i|, derived in tests/attention_ref.py from where the kernels round;
tests/test_attention_bound_cpu.py shows that rounding alone stays inside them.

Worst |got - ref| / bound measured on an MI355X (256 CUs), over all cases of a variant (every case prints its own line):

    forward (keys of tests/attention_census.py)        dh 64: ctx   lse2     dh 32: ctx   lse2
    plain FULL + KVNT   (seq_len 512)                        0.91  0.03            0.81  0.04
    plain FULL          (seq_len 1024)                       0.80  0.03            0.91  0.03
    plain key-bound     (528 / 784 / 2096)                   0.85  0.04            0.83  0.05
    pre-scaled KVNT     (512)                                0.84   -              0.84   -
    pre-scaled          (1024)                               0.80   -              0.89   -
    dropout generator, 8 waves                               0.88  0.03            0.80  0.04
    dropout bit reader, key-bound                            0.84  0.04            0.86  0.05
    dropout bit reader, FULL                                 0.83  0.03             (no such build)

    backward <dh, DROP, FULL>, row-major | panel       D            dQ           dK           dV
    <64, 0, 1>                                         0.02 | 0.02  0.61 | 0.63  0.31 | 0.35  0.45 | 0.33
    <64, 0, 0>                                         0.02 | 0.02  0.59 | 0.63  0.31 | 0.43  0.29 | 0.42
    <64, 1, 1>                                         0.03 | 0.02  0.63 | 0.60  0.37 | 0.36  0.42 | 0.37
    <64, 1, 0>                                         0.02 | 0.02  0.65 | 0.61  0.38 | 0.32  0.44 | 0.36
    <32, 0, 1>                                         0.04 | 0.04  0.66 | 0.62  0.41 | 0.31  0.36 | 0.34
    <32, 0, 0>                                         0.05 | 0.05  0.64 | 0.69  0.28 | 0.42  0.37 | 0.38
    <32, 1, 1>                                         0.04 | 0.04  0.69 | 0.63  0.46 | 0.27  0.42 | 0.34
    <32, 1, 0>                                         0.05 | 0.05  0.68 | 0.63  0.38 | 0.27  0.44 | 0.29
    forward -> backward chained (its own wider bounds) 0.04         0.32         0.09         0.32

No variant needed a term beyond the derived bounds.  The forward's 0.8 - 0.9 stands against 0.5 - 0.6 of the CPU emulation; the two are
not the same experiment (a multi-item case takes the maximum over some hundred times more elements than the emulation's three (batch,
head)s, and the kernels add the hardware exp2, the lazily updated running reference and their own summation order), and the shares of
these have not been separated."""
import ctypes as C
import functools
import math

import pytest
import torch

import attention_census as ac
import attention_ref as ar

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import check, current_stream, lib  # noqa: E402
from test_dropout_gpu import bits_to_mask  # noqa: E402
from test_gemm_matrix_gpu import DEV, Operand, _vt_perm, close  # noqa: E402

NAN = float("nan")
SENTINEL = 0x5A5A5A5A
SLACK = 256


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def multi_shape(slots, per_bh, nh):
    """(B, grid) for a persistent launch of B nh per_bh items = 2 slots + r, 0 < r < slots"""
    target = 2 * slots + slots // 8 + 1
    B = -(-target // (nh * per_bh))
    n = B * nh * per_bh
    assert 2 * slots < n < 3 * slots, (n, slots)
    return B, slots


def hot_items(grid, per_bh, n):
    """(batch, head)s of items a block walks second (index grid + bx) and third"""
    return tuple(sorted({min(n - 1, i // per_bh) for i in (grid + 1, grid + grid // 2, 2 * grid - 1, 2 * grid + 3)}))


@functools.lru_cache(maxsize=2)
def inputs(B, nh, L, dh, hot, pre):
    return ar.stress_inputs(B, nh, L, dh, seed=1000 + L + dh, hot=hot, pre=pre)


@functools.lru_cache(maxsize=2)
def plain_reference(B, nh, L, dh, hot, pre, bwd):
    """the reference of a case without dropout (cached: the variants and layouts of one shape share it)"""
    _, _, q, k, v, dO = inputs(B, nh, L, dh, hot, pre)
    return ar.reference(q, k, v, math.log(2.0) if pre else 1.0 / math.sqrt(dh), None, 0.0, dO if bwd else None)


def compare(case, name, got, ref, r):
    """one output against the reference, every element; prints the worst err / bound (the module docstring's table)"""
    rtol = ar.RTOL_F32 if name in ("D", "lse2") else ar.EPS
    want, atol = r[name].reshape(got.shape), r[name + "_atol"].reshape(got.shape)
    g = got.double().cpu()
    if bool(torch.isfinite(g).all()):
        print("ATTN-MATRIX %s %s %.3f" % (case, name, float(((g - want).abs() / (atol + rtol * want.abs())).max())))
    close("%s: %s" % (case, name), got, want, atol, rtol)


class RowsOut:
    """a [rows, cols] output, row-major with `pad` extra columns per row, NaN everywhere before the launch"""
    panel = 0

    def __init__(self, rows, cols, pad, dtype=torch.bfloat16):
        self.cols, self.ld = cols, cols + pad
        self.buf = torch.full((rows, self.ld), NAN, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr()

    def read(self):
        b = self.buf.cpu()
        assert bool(torch.isnan(b[:, self.cols:].float()).all()), "written into the pad columns"
        return b[:, :self.cols]


def vector_out(n):
    return torch.full((n + SLACK,), NAN, device=DEV)


def read_vector(t, n, what):
    t = t.cpu()
    assert bool(torch.isnan(t[n:]).all()), "%s: written behind its %d elements" % (what, n)
    return t[:n]


def heads_of(x, B, nh, L, dh):
    """token-major [B L, nh dh] -> [B nh, L, dh]"""
    return x.reshape(B, L, nh, dh).permute(0, 2, 1, 3).reshape(B * nh, L, dh)


def random_keep_words(n_words, p, seed):
    """int32 keep words whose bits are 1 with probability 1 - p (any bit pattern is a mask: what a test injects into the bit reader)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.arange(32, device=DEV, dtype=torch.int64)
    out = torch.empty(n_words, dtype=torch.int64, device=DEV)
    for a in range(0, n_words, 1 << 20):
        b = min(n_words, a + (1 << 20))
        out[a:b] = ((torch.rand(b - a, 32, device=DEV, generator=g) >= p).to(torch.int64) << w).sum(1)
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


class KeepBits:
    """the keep-bit tensor of B nh (batch, head)s with a sentinel behind it; `mask(a, b)` decodes (batch, head)s a..b - 1 on the host"""

    def __init__(self, n, L, p, words=None):
        self.n, self.L, self.p = n, L, p
        self.words = int(lib().mh_dropout_bits_words(n, L))
        self.buf = torch.full((self.words + 64,), SENTINEL, dtype=torch.int32, device=DEV)
        if words is not None:
            self.buf[:self.words] = words

    def mask(self, a, b):
        per = self.words // self.n
        return bits_to_mask(self.buf[a * per:b * per], b - a, self.L).cpu()

    def check_sentinel(self):
        assert bool((self.buf[self.words:] == SENTINEL).all()), "keep bits written behind mh_dropout_bits_words"


def dropout_desc(p, seed):
    d = _lib.Dropout()
    d.p, d.seed, d.offset, d.mask = p, 0x5DEECE66D ^ seed, (9 << 16) | (seed & 0xFFFF), None
    return d


def launched(case, recs, keys, multi):
    """the launch took the variant under test; a multi-item case really is one"""
    seen = {}
    for k, note, grid in recs:
        seen[k] = (note, grid)
    for key in keys:
        assert key in seen, "%s: the launch took %s, not the variant under test (%s)" % (case, sorted(seen), key)
        note, grid = seen[key]
        if multi:
            assert 2 * grid < ac.items(note) < 3 * grid, "%s: %s is no 2-to-3-items-per-block launch (grid %d)" % (case, note, grid)


# ------------------------------------------------------------------------------------------------------------------- forward
def forward_shape(kind, dh, L, shape, nh):
    """(B, nh, hot (batch, head)s) of a case; multi-item: from the CU count, the block's queries and the slots of the variant's geometry"""
    if shape != "multi":
        return 3, 5, ()
    small = kind == "gen"                               # the generator runs on 8 waves x 256 queries, two blocks per CU
    per_bh = -(-L // (256 if small else 512))
    B, grid = multi_shape(_cus() * (2 if small else 1), per_bh, nh)
    return B, nh, hot_items(grid, per_bh, B * nh)


def run_forward(case, kind, dh, L, shape, nh, tokens, panel, lse, p):
    """one streaming forward through the C ABI: kind plain (mh_attention_stream_fwd_ex), pre (_fwd_prescaled), gen / read (_fwd_drop:
    keep bits generated / read); q and k [B, nh, L, dh] or column blocks of the token-major projection; ctx row-major (pitch H + 8) or
    K32 panels in a row window"""
    B, nh, hot = forward_shape(kind, dh, L, shape, nh)
    n, H, pre = B * nh, nh * dh, kind == "pre"
    qkv, _, q, k, v, _ = inputs(B, nh, L, dh, hot, pre)
    scale = 1.0 / math.sqrt(dh)
    if tokens:
        qkv_d = qkv.to(DEV)
        qp, kp, strides = qkv_d.data_ptr(), qkv_d.data_ptr() + 2 * H, (L * 3 * H, dh, 3 * H)
    else:
        q_d, k_d = q.to(DEV).contiguous(), k.to(DEV).contiguous()
        qp, kp, strides = q_d.data_ptr(), k_d.data_ptr(), (nh * L * dh, L * dh, dh)
    vt = torch.zeros(n * dh * L + SLACK, dtype=torch.bfloat16, device=DEV)
    vt[:n * dh * L] = _vt_perm(v.transpose(1, 2).contiguous()).reshape(-1).to(DEV)
    # (seq_len 528: a pitch that is no multiple of 8 - the 8-byte store path)
    out = Operand(torch.empty(B * L, H), True, r0=64, extra=64, fill="nan") if panel else RowsOut(B * L, H, 4 if L == 528 else 8)
    lse2 = vector_out(n * L) if lse else None
    lp = lse2.data_ptr() if lse else None
    bits, d = None, None
    if kind in ("gen", "read"):
        d = dropout_desc(p, L + dh)
        bits = KeepBits(n, L, p, random_keep_words(int(lib().mh_dropout_bits_words(n, L)), p, L + dh) if kind == "read" else None)
    st, L_ = current_stream(), lib()
    if pre:
        assert not tokens and not lse
        run = lambda: check(L_.mh_attention_stream_fwd_prescaled(qp, kp, vt.data_ptr(), out.ptr, out.ld, out.panel, B, L, nh, dh, st))  # noqa: E731
    elif d is None:
        run = lambda: check(L_.mh_attention_stream_fwd_ex(qp, kp, vt.data_ptr(), out.ptr, out.ld, out.panel, B, L, nh, dh, scale, lp,  # noqa: E731
                                                          *strides, st))
    else:
        run = lambda: check(L_.mh_attention_stream_fwd_drop(qp, kp, vt.data_ptr(), out.ptr, out.ld, out.panel, B, L, nh, dh, scale, lp,  # noqa: E731
                                                            *strides, C.byref(d), bits.buf.data_ptr(), int(kind == "read"), st))
    recs = ac.record(run)
    full = L % 256 == 0
    key = {"plain": ac.fwd_key(dh, full=full, kvnt=full and L <= 512),
           "pre": ac.fwd_key(dh, full=1, kvnt=L <= 512, pre=1),
           "gen": ac.fwd_key(dh, nw=8, sk=128 if dh == 64 else 256, dropv=1),
           "read": ac.fwd_key(dh, dropv=2, full=full and dh == 64)}[kind]
    launched(case, recs, [key], shape == "multi")
    if bits is not None:
        bits.check_sentinel()
        if kind == "gen":       # the generator's words == the standalone kernel's (pinned to the host rule in test_round3_kernels_gpu.py)
            alone = torch.full((bits.words,), ~SENTINEL, dtype=torch.int32, device=DEV)
            check(L_.mh_dropout_bits(alone.data_ptr(), n, L, C.byref(d), st))
            assert torch.equal(bits.buf[:bits.words], alone), "%s: generated keep bits differ from mh_dropout_bits" % case
        r = ar.reference(q, k, v, scale, bits.mask, p)
    else:
        r = plain_reference(B, nh, L, dh, hot, pre, False)
    compare(case, "ctx", heads_of(out.read(), B, nh, L, dh), r["ctx"], r)
    if lse:
        compare(case, "lse2", read_vector(lse2, n * L, "lse2").view(n, L), r["lse2"], r)


def _fwd_cases():
    out = []
    for dh in (64, 32):
        nh = 5 if dh == 64 else 6
        cases = [
            # (variant, kind, L, shape, tokens, panel, lse, p)
            ("plain-full-kvnt", "plain", 512, "small", 0, 0, 1, 0), ("plain-full-kvnt", "plain", 512, "multi", 1, 1, 1, 0),
            ("plain-full", "plain", 1024, "small", 1, 0, 0, 0), ("plain-full", "plain", 1024, "multi", 0, 1, 1, 0),
            ("plain-bound", "plain", 528, "ragged", 1, 0, 1, 0), ("plain-bound", "plain", 784, "ragged", 0, 1, 0, 0),
            ("plain-bound", "plain", 2096, "ragged", 1, 1, 1, 0), ("plain-bound", "plain", 528, "multi", 1, 0, 1, 0),
            ("pre-kvnt", "pre", 512, "small", 0, 0, 0, 0), ("pre-kvnt", "pre", 512, "multi", 0, 1, 0, 0),
            ("pre", "pre", 1024, "small", 0, 1, 0, 0), ("pre", "pre", 1024, "multi", 0, 0, 0, 0),
            ("drop-gen", "gen", 528, "ragged", 1, 0, 1, 0.1), ("drop-gen", "gen", 784, "ragged", 0, 1, 1, 0.5),
            ("drop-gen", "gen", 1024, "small", 1, 1, 1, 0.1), ("drop-gen", "gen", 512, "multi", 1, 0, 1, 0.1),
            ("drop-read-bound", "read", 528, "ragged", 1, 1, 1, 0.1), ("drop-read-bound", "read", 2096, "ragged", 1, 0, 1, 0.1),
            ("drop-read-bound", "read", 528, "multi", 1, 0, 1, 0.1),
        ]
        if dh == 64:
            # (seq_len 1024 in the multi-item regime: what the training step launches)
            cases += [("drop-read-full", "read", 1024, "small", 1, 0, 1, 0.1), ("drop-read-full", "read", 1024, "multi", 1, 1, 1, 0.1)]
        else:           # head dim 32: the bit reader has no bound-free build - whole-stage lengths run the key-bound one
            cases += [("drop-read-bound", "read", 1024, "small", 1, 0, 1, 0.1), ("drop-read-bound", "read", 512, "multi", 1, 1, 1, 0.1)]
        for variant, kind, L, shape, tokens, panel, lse, p in cases:
            cid = "%s-dh%d-%s-L%d-%s-%s%s%s" % (variant, dh, shape, L, "tokens" if tokens else "heads", "panel" if panel else "rows",
                                                 "-lse" if lse else "", "-p%g" % p if p else "")
            out.append(pytest.param(kind, dh, L, shape, nh, tokens, panel, lse, p, id=cid))
    return out


@pytest.mark.parametrize("kind,dh,L,shape,nh,tokens,panel,lse,p", _fwd_cases())
def test_forward_variant_against_reference(request, kind, dh, L, shape, nh, tokens, panel, lse, p):
    run_forward(request.node.callspec.id, kind, dh, L, shape, nh, tokens, panel, lse, p)


# ------------------------------------------------------------------------------------------------------------------ backward
def run_backward(case, dh, L, shape, nh, tokens, panel, p, chained=False):
    """dQ, dK, dV and D of mh_attention_stream_bwd_layout: q / k / v / dO (and row-major O) [B, nh, L, dh] or token-major column blocks; O as
    K32 panels in a row window and dQ | dK | dV as the three column blocks of one panel buffer (panel: what the fused training layer
    passes), or O in dO's row layout and dQ | dK | dV column blocks of a token-major [B L, 3 H + 8] buffer"""
    if shape == "multi":
        per_bh = -(-L // 256)
        B, grid = multi_shape(_cus(), per_bh, nh)
        hot = hot_items(grid, per_bh, B * nh)
    else:
        B, nh, hot = 3, 5, ()
    n, H = B * nh, nh * dh
    qkv, dctx, q, k, v, dO = inputs(B, nh, L, dh, hot, False)
    scale = 1.0 / math.sqrt(dh)
    st, L_ = current_stream(), lib()
    bits = KeepBits(n, L, p, random_keep_words(int(lib().mh_dropout_bits_words(n, L)), p, 7 * L + dh)) if p else None
    if chained:
        # the forward kernel's own O and lse2 (fp32), as training chains them.  O then differs from the exact rows by up to the forward's
        # tolerance, not by one rounding: D's error bound grows to sum_d |dO| (atol_ctx + EPS |O|), and lse2's tolerance scales P by
        # 2^(its error): ln 2 x that tolerance joins EPS in the dS terms (tests/attention_ref.py: reference(chained=True))
        assert tokens and not p
        qkv_d = qkv.to(DEV)
        vt = torch.zeros(n * dh * L + SLACK, dtype=torch.bfloat16, device=DEV)
        vt[:n * dh * L] = _vt_perm(v.transpose(1, 2).contiguous()).reshape(-1).to(DEV)
        o_rows, lse_d = torch.empty(B * L, H, dtype=torch.bfloat16, device=DEV), torch.empty(n * L, device=DEV)
        check(L_.mh_attention_stream_fwd_ex(qkv_d.data_ptr(), qkv_d.data_ptr() + 2 * H, vt.data_ptr(), o_rows.data_ptr(), H, 0, B, L, nh, dh, scale,
                                            lse_d.data_ptr(), L * 3 * H, dh, 3 * H, st))
        o_tok = o_rows.cpu()
        r = ar.reference(q, k, v, scale, None, 0.0, dO, chained=True)
        og = dO.double() * heads_of(o_tok, B, nh, L, dh).double()
        r["D"], r["D_atol"] = og.sum(-1), dh * 2.0 ** -24 * og.abs().sum(-1)
    else:
        r = ar.reference(q, k, v, scale, bits.mask, p, dO) if p else plain_reference(B, nh, L, dh, hot, False, True)
        o_tok = r["o_given"].view(B, nh, L, dh).permute(0, 2, 1, 3).reshape(B * L, H).bfloat16()
        lse_d = r["lse2_given"].reshape(-1).float().to(DEV)
    if tokens:
        if not chained:
            qkv_d = qkv.to(DEV)
        dctx_d = dctx.to(DEV)
        qp, kp, vp, dop = qkv_d.data_ptr(), qkv_d.data_ptr() + 2 * H, qkv_d.data_ptr() + 4 * H, dctx_d.data_ptr()
        lqkv, ldo = (L * 3 * H, dh, 3 * H), (L * H, dh, H)
        o_d = o_tok.to(DEV)
    else:
        q_d, k_d, v_d, dO_d = (t.to(DEV).contiguous() for t in (q, k, v, dO))
        qp, kp, vp, dop = q_d.data_ptr(), k_d.data_ptr(), v_d.data_ptr(), dO_d.data_ptr()
        lqkv = ldo = (nh * L * dh, L * dh, dh)
        o_d = heads_of(o_tok, B, nh, L, dh).contiguous().to(DEV)
    if panel:
        Oo = Operand(o_tok, True, r0=96, extra=32)
        op, o_ld = Oo.ptr, Oo.ld
        G = Operand(torch.empty(B * L, 3 * H), True, r0=64, extra=64, fill="nan")
        blk = (H // 32) * G.ld * 32 * 2                                   # bytes of one of the three column blocks in panel form
        dqp, dkp, dvp = G.ptr, G.ptr + blk, G.ptr + 2 * blk
    else:
        op, o_ld = o_d.data_ptr(), 0
        G = RowsOut(B * L, 3 * H, 8)
        dqp, dkp, dvp = G.ptr, G.ptr + 2 * H, G.ptr + 4 * H
    D = vector_out(n * L)
    recs = ac.record(lambda: check(L_.mh_attention_stream_bwd_layout(
        qp, kp, vp, dop, op, int(panel), o_ld, lse_d.data_ptr(), D.data_ptr(), dqp, dkp, dvp, G.ld, int(panel), B, L, nh, dh, scale, *lqkv, *ldo,
        bits.buf.data_ptr() if p else None, p, st)))
    launched(case, recs, ac.bwd_keys(dh, p > 0, L % 256 == 0, panel), shape == "multi")
    if bits is not None:
        bits.check_sentinel()
    compare(case, "D", read_vector(D, n * L, "D").view(n, L), r["D"], r)
    g = G.read()
    for i, name in enumerate(("dq", "dk", "dv")):
        compare(case, name, heads_of(g[:, i * H:(i + 1) * H], B, nh, L, dh), r[name], r)


def _bwd_cases():
    out = []
    for dh in (64, 32):
        nh = 3 if dh == 64 else 6
        for p in (0.0, 0.1):
            cases = [
                # (L, shape, tokens, panel, p): FULL builds (seq_len % 256 == 0) ...
                (512, "small", 0, 0, p), (1024, "small", 1, 1, p), (512, "multi", 1, 0, p),
                # ... and the key-bound ones
                (528, "ragged", 0, 0, p), (784, "ragged", 1, 1, 0.5 if p and dh == 64 else p), (2096, "ragged", 1, int(p > 0), p),
                (528, "multi", 1, int(p == 0), p),
            ]
            if dh == 64:      # (four items per block with panel operands: what the fused training layer launches)
                cases.append((1024, "multi", 1, 1, p))
            for L, shape, tokens, panel, pp in cases:
                cid = "dh%d-%s-%s-%s-L%d-%s-%s%s" % (dh, "drop" if p else "plain", "full" if L % 256 == 0 else "bound", shape, L,
                                                      "tokens" if tokens else "heads", "panel" if panel else "rows", "-p%g" % pp if pp else "")
                out.append(pytest.param(dh, L, shape, nh, tokens, panel, pp, id=cid))
    return out


@pytest.mark.parametrize("dh,L,shape,nh,tokens,panel,p", _bwd_cases())
def test_backward_variant_against_reference(request, dh, L, shape, nh, tokens, panel, p):
    run_backward(request.node.callspec.id, dh, L, shape, nh, tokens, panel, p)


@pytest.mark.parametrize("dh,L", [(64, 784), (32, 1024)])
def test_forward_then_backward_chained(request, dh, L):
    """forward kernel -> backward kernels on the forward's own O and lse2, as training runs them (token-major operands, panel gradients)"""
    run_backward("chained-" + request.node.callspec.id, dh, L, "small", 5, 1, 1, 0.0, chained=True)
