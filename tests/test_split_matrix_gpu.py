"""Parity matrix of the split-precision kernels (csrc/split.hip): every C entry point called through the library's ABI against a float64
reference on the CPU (tests/split_ref.py), EVERY element of EVERY output, in both part types, at the smallest shapes at which each path
of a kernel exists - K = 32 (two DMA stages: prologue and peeled stages only), K = 64 (the first in-loop issue inside the peeled even
stage), K = 96; ragged M and N in every output form; a persistent launch whose tile count leaves mh_xcd_remap a remainder and whose
fast and guarded epilogues both run after a prefetch and without one; the non-temporal stores; operands that are row windows of larger
buffers, the stacked q | k | v weight of the V^T projection exactly as csrc/engine.hip passes it; one key tile with 56 masked keys, a last
key tile of 8 keys, the first 8-wave launch, the half-empty d tile of head dim 16; LayerNorm rows with four active lanes, a lane-dependent
last chunk round, waves that own no row.

Rules of every case: operands are built on the host from parts that tests/split_ref.py rounds itself (the pack kernel is a case of its
own, not a helper); every output buffer starts as NaN with pitch columns, pad rows and SLACK elements behind its end, and whatever lies
outside the documented output must still be NaN afterwards (the pack kernel's K padding, columns cols .. kpad, must be zero); pad rows of
A, W and the residual, the gaps between parts and whatever lies around a row window are NaN; the comparison is |got - ref| <= bound per
element with got = hi + lo; the exact movers are compared bit for bit: pack (hi = the value rounded to the 16-bit type, lo = the rounded
remainder) and join (fp32 hi + lo).  Every case records its launch (tests/split_census.py) and asserts the census key it ran, which is
what tests/test_split_census_gpu.py's PARITY table is generated from.

What the pack kernel does with values outside the fp16 range, tested exactly: fp16 parts saturate, so 1e6, +inf and every value above
65504 store hi = 65504, lo = 0 (negative: -65504, -0); 65519 (below the rounding boundary 65520) stores the same.  bf16 parts do not
saturate: 1e6 stores its two parts, +-inf stores hi = +-inf and lo = NaN (inf - inf).

The one case that samples: the non-temporal-store launches (`stream`: M N 4 bytes just above 192 MiB, N = 2048) compare the rows of the
first tile, of the last tile and every 97th row with the reference - a float64 product of all 50 M elements takes longer than the rest
of the module together - and check on the device that every other element of the output was written and nothing behind it was.

Worst |got - ref| / bound per output and part type, measured on an MI355X over all cases of a test (every case prints its own
SPLIT-MATRIX line):

    output                                   bf16x3   f16x3
    pack hi | lo | K padding, join rows       exact    exact
    layernorm           y                     0.45     0.48
    GEMM                K = 32                0.46     0.20
                        K = 64                0.26     0.22
                        K = 96                0.24     0.21
                        persistent            0.43     0.11
                        non-temporal stores   0.43     0.31
    dense + residual + LayerNorm  y           0.32     0.03
    attention  ctx      dh 16                 0.28     0.04
                        dh 32                 0.29     0.03
                        dh 64                 0.33     0.03
                        underflow (x250)      0.44     0.14

The bounds are worst-case (n u per sum, MATH_ULP ulp per function), hence the distance; the bf16x3 column sits higher because its
largest term, the parts' own 2^-16 (2^-15 for the truncated probabilities), is nearly reached by single elements.  No output needed a
term beyond the derived bounds.  Run time on the MI355X: 276 cases in 20 s; the slowest is persistent-grid-k32 (1.3 s), each
non-temporal-store case stays under 0.4 s with its row sample."""
import math

import numpy as np
import pytest
import torch

import split_census as sc
import split_ref as sr

pytestmark = pytest.mark.gpu

from musediffusion_amd._lib import MH_BF16X3, MH_F16X3, check, current_stream, lib  # noqa: E402

assert (MH_BF16X3, MH_F16X3) == (sr.BF16X3, sr.F16X3)
DEV = "cuda"
NAN = float("nan")
SLACK = 256
T16 = {sr.BF16X3: torch.bfloat16, sr.F16X3: torch.float16}
DT = pytest.mark.parametrize("dt", sr.DTYPES, ids=[sr.NAME[d] for d in sr.DTYPES])
f32 = np.float32
NT_BYTES = 192 << 20          # mh_split_gemm: non-temporal stores above this many bytes of M N 4


# ------------------------------------------------------------------------------------------------------------------ buffers
def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(DEV)


def dev16(a, dt):
    """float32 values that the 16-bit type holds exactly (or NaN / inf) -> device tensor of that type, flat, SLACK NaN elements behind"""
    t = torch.full((a.size + SLACK,), NAN, dtype=T16[dt], device=DEV)
    t[:a.size] = dev32(a).reshape(-1).to(T16[dt])
    return t


def nans(n, dtype=torch.float32):
    return torch.full((int(n) + SLACK,), NAN, dtype=dtype, device=DEV)


def host(t):
    return t.float().cpu().numpy()


def tail_is_nan(a, n, what):
    assert np.isnan(a[n:]).all(), "%s: written behind its %d elements" % (what, n)
    return a[:n]


def same(a, b):
    """bit for bit up to the payload of a NaN"""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def exact(case, name, got, want):
    ok = same(got, want)
    assert ok.all(), "%s %s: %d of %d elements differ, first at %s: got %r want %r" % (
        case, name, int((~ok).sum()), ok.size, np.unravel_index(int(np.argmin(ok)), ok.shape), got[~ok][0], want[~ok][0])


def compare(case, dt, name, got, pair):
    """hi + lo (or fp32 rows) against (ref, bound), every element; prints the worst err / bound (the module docstring's table)"""
    ref, bound = pair
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), "%s %s: %d elements never written (still NaN) or not finite, first at %s" % (
        case, name, int(bad.sum()), np.unravel_index(int(np.argmax(bad)), ref.shape))
    print("SPLIT-MATRIX %s %s %s %.3f" % (case, sr.NAME[dt], name, sr.ratio(got, ref, bound)))
    err = np.abs(got - ref)
    out = err > bound
    if out.any():
        i = np.unravel_index(int(np.argmax(err - bound)), ref.shape)
        pytest.fail("%s %s %s: %d of %d elements outside their bound; worst at %s: got %.9g ref %.9g (bound %.3g); first bad rows %s, columns %s"
                    % (case, sr.NAME[dt], name, int(out.sum()), out.size, i, got[i], ref[i], bound[i],
                       sorted(set(np.nonzero(out)[0].tolist()))[:8], sorted(set(np.nonzero(out)[-1].tolist()))[:8]))


def panel_operand(parts, dt, ld, r0=0):
    """parts [rows, cols] -> (tensor, pointer): split panels [2][cols / 32][ld][32] with the operand's rows at r0 .. r0 + rows of each
    (part, panel) and NaN in every other row - a row window of a larger buffer when r0 > 0; the pointer is that of row r0"""
    rows = parts[0].shape[0]
    assert r0 + rows <= ld
    pan = np.full((2, parts[0].shape[1] // 32, ld, 32), np.nan, dtype=f32)
    pan[:, :, r0:r0 + rows, :] = sr.to_panels(parts, rows)
    t = dev16(pan, dt)
    return t, t.data_ptr() + r0 * 32 * 2


def read_panels(t, dt, rows, cols, ld, what):
    """(hi, lo) [rows, cols] out of a NaN-initialised panel buffer [2][cols / 32][ld][32]; pad rows and the tail must still be NaN"""
    n = 2 * (cols // 32) * ld * 32
    pan = tail_is_nan(host(t), n, what).reshape(2, cols // 32, ld, 32)
    assert np.isnan(pan[:, :, rows:, :]).all(), "%s: written into panel rows behind row %d" % (what, rows)
    return sr.from_panels(pan, rows, cols)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------------ pack and join
# (rows, cols, extra panels of K padding)
MOVER_CASES = [(r, c, 2 if (r, c) == (63, 33) else 0) for r in (1, 63, 64, 200) for c in (1, 33, 70, 72)]


def _mover_id(c):
    return "r%d-c%d-pad%d" % (c[0], c[1], (c[1] + 31) // 32 * 32 + 32 * c[2])


@DT
@pytest.mark.parametrize("case", MOVER_CASES, ids=_mover_id)
def test_pack_bit_for_bit(case, dt):
    rows, cols, extra = case
    kpad, ldx, ld = (cols + 31) // 32 * 32 + 32 * extra, cols + 3, rows + 5
    x = sr.pack_inputs(rows, cols, dt, seed=rows * 100 + cols)
    xb = np.full((rows, ldx), np.nan, dtype=f32)
    xb[:, :cols] = x
    xd, out = dev32(xb), nans(2 * (kpad // 32) * ld * 32, T16[dt])
    keys = sc.keys_of(lambda: check(lib().mh_split_pack(xd.data_ptr(), ldx, out.data_ptr(), ld, rows, cols, kpad, dt, current_stream()), "mh_split_pack"))
    assert keys == [sc.mover_key("pack", sr.NAME[dt], cols)], keys
    hi, lo = read_panels(out, dt, rows, kpad, ld, "pack")
    want_hi, want_lo = sr.split_rn(x, dt)
    name = _mover_id(case)
    exact(name, "hi", hi[:, :cols], want_hi)
    exact(name, "lo", lo[:, :cols], want_lo)
    exact(name, "K padding", np.stack([hi[:, cols:], lo[:, cols:]]), np.zeros((2, rows, kpad - cols), dtype=f32))
    # the documented treatment of values outside the fp16 range (the module docstring), on the values themselves
    flat_hi, flat_lo, n = hi[:, :cols].reshape(-1), lo[:, :cols].reshape(-1), rows * cols
    if n >= 7:
        if dt == sr.F16X3:
            assert list(flat_hi[:7]) == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0] and not flat_lo[:7].any()
        else:
            assert flat_hi[5] == np.inf and flat_hi[6] == -np.inf and np.isnan(flat_lo[5:7]).all()
            assert float(flat_hi[3]) + float(flat_lo[3]) == pytest.approx(1e6, rel=2.0 ** -16) and flat_hi[0] == 65536.0
    if n >= 9 and dt == sr.F16X3:
        assert flat_hi[7] + flat_lo[7] != flat_hi[7] and abs(float(flat_lo[7])) < 2.0 ** -14          # a subnormal lo part is kept


@DT
@pytest.mark.parametrize("case", MOVER_CASES, ids=_mover_id)
def test_join_bit_for_bit(case, dt):
    rows, cols, extra = case
    cpad, ldo, ld = (cols + 31) // 32 * 32 + 32 * extra, cols + 3, rows + 5
    parts = sr.split_rn(sr.pack_inputs(rows, cpad, dt, seed=rows * 100 + cols + 7), dt)          # (the K padding holds values too: never copied)
    src, ptr = panel_operand(parts, dt, ld)
    out = nans(rows * ldo)
    keys = sc.keys_of(lambda: check(lib().mh_split_join(ptr, ld, out.data_ptr(), ldo, rows, cols, cpad, dt, current_stream()), "mh_split_join"))
    assert keys == [sc.mover_key("join", sr.NAME[dt], cols)], keys
    body = tail_is_nan(host(out), rows * ldo, "join").reshape(rows, ldo)
    assert np.isnan(body[:, cols:]).all(), "join: written into its pitch columns"
    want = sr.join(parts)[:, :cols]
    live = ~np.isnan(want)          # (bf16 parts of +-inf: hi + lo = NaN, which the NaN-filled buffer cannot tell from unwritten)
    exact(_mover_id(case), "rows", np.where(live, body[:, :cols], 0), np.where(live, want, 0))


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
# (H, rows, L, add: 2 = position / time rows with emb_row, 1 = with emb_row null (the batch index is the row), 0 = off; ldx - H)
LN_CASES = [(H, (1, 5, 72)[(i + a) % 3], (1, 5, 24)[(i + a) % 3], a, 4 * ((i + a) % 2))
            for i, H in enumerate((32, 512, 544, 1024, 1056, 2048)) for a in (2, 1, 0)]


def _ln_id(c):
    return "H%d-r%d-L%d-%s-ldx+%d" % (c[0], c[1], c[2], ("off", "add-batchrow", "add-embrow")[c[3]], c[4])


def ln_case(case):
    H, rows, L, add, dx = case
    x, gamma, beta = sr.ln_inputs(rows, H, seed=H + rows + add)
    g = sr.rng(H * 3 + add)
    B = rows // L
    pos = g.standard_normal((L, H)).astype(f32) if add else None
    emb = g.standard_normal((B + 2, H)).astype(f32) if add else None
    rows_of = ((np.arange(B) * 2 + 1) % (B + 2)).astype(np.int32) if add == 2 else np.arange(B, dtype=np.int32)
    return x, gamma, beta, pos, emb, rows_of


@DT
@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm(case, dt):
    H, rows, L, add, dx = case
    x, gamma, beta, pos, emb, rows_of = ln_case(case)
    eps, ldx, ld = 1e-12, H + dx, rows + 3
    xb = np.full((rows, ldx), np.nan, dtype=f32)
    xb[:, :H] = x
    xd, gd, bd = dev32(xb), dev32(gamma), dev32(beta)
    pd, ed, rd = (dev32(pos), dev32(emb), torch.from_numpy(rows_of).to(DEV)) if add else (None, None, None)
    out = nans(2 * (H // 32) * ld * 32, T16[dt])
    keys = sc.keys_of(lambda: check(lib().mh_split_layernorm(
        xd.data_ptr(), ldx, pd.data_ptr() if add else None, ed.data_ptr() if add else None, rd.data_ptr() if add == 2 else None, gd.data_ptr(),
        bd.data_ptr(), out.data_ptr(), ld, rows, L, H, eps, dt, current_stream()), "mh_split_layernorm"))
    assert keys == [sc.ln_key(sr.NAME[dt], add, H)], keys
    compare(_ln_id(case), dt, "y", sr.val(read_panels(out, dt, rows, H, ld, "layernorm")),
            sr.layernorm(x, pos, emb, rows_of, L, gamma, beta, eps, dt))


# ------------------------------------------------------------------------------------------------------------------ GEMM
NONE, TANH, GELU = sr.ACT_NONE, sr.ACT_TANH, sr.ACT_GELU
# (id, M, N, K, act, out_mode, bias "0" / "col" / "row", residual, form).  form: "pitch" (every pitch larger than its rows, NaN pad rows),
# "window" (A and W row windows of larger buffers), "vt" (the V^T projection of csrc/engine.hip: A = rows 2H .. of the stacked weight),
# "thin" (persistent: one column tile, more row tiles than blocks), "grid" (persistent: 17 column tiles, ragged in M and N, a tile count
# that is no multiple of 8), "stream" (the non-temporal stores; rows sampled).  M None: derived from the device's CU count.
GEMM_CASES = [
    ("k32-panels", 300, 160, 32, TANH, 0, "col", 1, "pitch"),
    ("k32-rows16", 300, 72, 32, NONE, 1, "row", 0, "pitch"),
    ("k32-f32", 1, 3, 32, GELU, 2, "0", 0, "pitch"),
    ("k32-f32-wide", 300, 500, 32, NONE, 2, "col", 0, "window"),
    ("k64-panels", 300, 160, 64, GELU, 0, "col", 0, "window"),
    ("k64-rows16", 1, 72, 64, TANH, 1, "0", 0, "pitch"),
    ("k64-f32", 300, 500, 64, NONE, 2, "row", 0, "pitch"),
    ("k64-f32-res", 300, 160, 64, NONE, 2, "col", 1, "pitch"),
    ("k96-panels-rowbias", 300, 160, 96, NONE, 0, "row", 1, "pitch"),
    ("k96-rows16-gelu", 300, 72, 96, GELU, 1, "col", 0, "pitch"),
    ("k96-f32-tanh", 300, 500, 96, TANH, 2, "col", 0, "pitch"),
    ("k96-f32-n3", 300, 3, 96, NONE, 2, "col", 0, "pitch"),
    ("k96-panels-tanh", 600, 160, 96, TANH, 0, "col", 0, "pitch"),
    ("k96-panels-gelu", 300, 160, 96, GELU, 0, "col", 0, "pitch"),
    ("k96-rows16-window", 300, 72, 96, NONE, 1, "col", 0, "window"),
    ("k96-f32-res", 300, 160, 96, NONE, 2, "col", 1, "pitch"),
    ("k96-vt-stacked", 64, 200, 96, NONE, 1, "row", 0, "vt"),
    ("persistent-grid-k32", None, 2144, 32, NONE, 0, "col", 1, "grid"),
    ("persistent-tanh-panels", None, 32, 96, TANH, 0, "col", 0, "thin"),
    ("persistent-gelu-panels", None, 32, 96, GELU, 0, "col", 0, "thin"),          # (FFN1 of a batch slice: below the non-temporal threshold)
    ("persistent-f32", None, 3, 96, NONE, 2, "col", 0, "thin"),
    ("persistent-f32-res", None, 32, 96, NONE, 2, "col", 1, "thin"),
    ("persistent-rows16", None, 8, 96, NONE, 1, "col", 0, "thin"),
    ("persistent-rows16-rowbias", None, 8, 96, NONE, 1, "row", 0, "thin"),
    ("stream-k32", NT_BYTES // (2048 * 4) + 1, 2048, 32, GELU, 0, "col", 0, "stream"),
    ("stream-k96", NT_BYTES // (2048 * 4) + 1, 2048, 96, GELU, 0, "col", 0, "stream"),
]
PERSISTENT = ("grid", "thin", "stream")


def _gemm_id(c):
    return c[0]


def gemm_case_key(case, dt):
    """the census key a GEMM case launches (asserted by the case itself)"""
    name, M, N, K, act, out, bias, res, form = case
    return sc.gemm_key(sr.NAME[dt], act, out, bias, res, form == "stream", form in PERSISTENT, K)


def gemm_rows(case, n_cus=None):
    """M of a case whose row count depends on the device: more tiles than the 2 blocks per CU of a persistent launch"""
    name, M, N, K, act, out, bias, res, form = case
    if M is not None:
        return M
    slots = 2 * (n_cus or cus())
    if form == "thin":
        return 256 * (slots + 3) - 40
    tiles_m = -(-(slots + 1) // 17) + 2
    if (tiles_m * 17) % 8 == 0:
        tiles_m += 1
    return 256 * tiles_m - 100


def stream_rows(M):
    """the rows the non-temporal-store case compares: the first tile, the last tile, every 97th row"""
    return np.unique(np.concatenate([np.arange(min(256, M)), np.arange((M - 1) // 256 * 256, M), np.arange(0, M, 97)]))


def gemm_operands(case, M, dt):
    name, _, N, K, act, out_mode, bias, res, form = case
    seed = sum(map(ord, name))
    A, W = sr.values((M, K), dt, seed, 0.7), sr.values((N, K), dt, seed + 1, 1.5 / math.sqrt(K))
    bias_v = (0.3 * sr.rng(seed + 2).standard_normal(M if bias == "row" else N)).astype(f32) if bias != "0" else None
    R = sr.values((M, N), dt, seed + 3) if res else None
    return A, W, bias_v, R


@DT
@pytest.mark.parametrize("case", GEMM_CASES, ids=_gemm_id)
def test_gemm(case, dt):
    name, _, N, K, act, out_mode, bias, res, form = case
    M = gemm_rows(case)
    tiles = -(-M // 256) * -(-N // 128)
    assert (tiles > 2 * cus()) == (form in PERSISTENT), (tiles, cus())
    if form == "grid":
        assert tiles % 8 != 0 and M % 256 != 0 and N % 128 != 0
    seed = sum(map(ord, name))
    A, W, bias_v, R = gemm_operands(case, M, dt)
    if form == "vt":
        # csrc/engine.hip: mh_split_gemm(w_qkv + 2H rows, 3H, X, N, b_qkv + 2H, 1, ..., vt, N, 1, H N, H, N, H, ...): the stacked weight
        # [2][K / 32][3H][32] with NaN-free q | k rows in front of the window and nothing but the buffer's end behind it
        H = M
        stack = tuple(np.concatenate([sr.values((2 * H, K), dt, seed + 4, 0.5)[p], A[p]]) for p in range(2))
        At, a_ptr = panel_operand(stack, dt, 3 * H)
        a_ptr, lda = a_ptr + 2 * H * 32 * 2, 3 * H
        Wt, w_ptr = panel_operand(W, dt, N)
        ldw = N
        bt = dev32(np.concatenate([np.full(2 * H, np.nan, dtype=f32), bias_v]))
        b_ptr = bt.data_ptr() + 2 * H * 4
    else:
        r0 = 5 if form == "window" else 0
        lda, ldw = r0 + M + 7, r0 + N + 9
        At, a_ptr = panel_operand(A, dt, lda, r0)
        Wt, w_ptr = panel_operand(W, dt, ldw, r0)
        bt = dev32(bias_v) if bias != "0" else None
        b_ptr = bt.data_ptr() if bias != "0" else None
    ldr = M + 5
    Rt, r_ptr = panel_operand(R, dt, ldr) if res else (None, None)
    if out_mode == 0:
        ldo, part = M + 3, 0
        out = nans(2 * (N // 32) * ldo * 32, T16[dt])
    elif out_mode == 1:
        ldo = N if form == "vt" else N + 8
        part = M * ldo + (0 if form == "vt" else 16)
        out = nans(part + M * ldo, T16[dt])
    else:
        ldo, part = (N + 3) // 4 * 4 + 4, 0
        out = nans(M * ldo)
    keys = sc.keys_of(lambda: check(lib().mh_split_gemm(a_ptr, lda, w_ptr, ldw, b_ptr, int(bias == "row"), r_ptr, ldr if res else 0, out.data_ptr(), ldo,
                                                        out_mode, part, M, N, K, act, dt, current_stream()), "mh_split_gemm"))
    assert keys == [gemm_case_key(case, dt)], keys
    rows = stream_rows(M) if form == "stream" else np.arange(M)
    if form == "stream":
        # every element of every row written, nothing behind the rows or the buffer (on the device: 100 M elements); the values of `rows`
        pan = out[:2 * (N // 32) * ldo * 32].view(2, N // 32, ldo, 32)
        assert bool(torch.isfinite(pan[:, :, :M, :]).all()) and bool(torch.isnan(pan[:, :, M:, :]).all()) and bool(torch.isnan(out[pan.numel():]).all())
        sub = host(pan[:, :, torch.from_numpy(rows).to(DEV), :])
        got = sr.val(sr.from_panels(sub, rows.size, N))
    elif out_mode == 0:
        got = sr.val(read_panels(out, dt, M, N, ldo, "out"))
    elif out_mode == 1:
        a = tail_is_nan(host(out), part + M * ldo, "out")
        hi, lo = a[:M * ldo].reshape(M, ldo), a[part:].reshape(M, ldo)
        assert np.isnan(hi[:, N:]).all() and np.isnan(lo[:, N:]).all() and np.isnan(a[M * ldo:part]).all(), "written outside the two [M, N] parts"
        got = sr.val((hi[:, :N], lo[:, :N]))
    else:
        body = tail_is_nan(host(out), M * ldo, "out").reshape(M, ldo)
        assert np.isnan(body[:, N:]).all(), "written into the pitch columns"
        got = body[:, :N]
    sel = lambda P: tuple(p[rows] for p in P) if P is not None else None
    ref = sr.gemm(sel(A), W, bias_v if bias == "col" else None, bias_v[rows] if bias == "row" else None, act, sel(R), out_mode, dt)
    compare(name, dt, "out", got, ref)


# ------------------------------------------------------------------------------------------------------------------ dense + residual + LayerNorm
GEMM_LN_CASES = [(32, 8), (32, 1000), (64, 128), (64, 129), (96, 129), (96, 1000), (2048, 8), (2048, 128)]


def gemm_ln_case(K, M, dt):
    """operands of a full-row case: the bias in eighths, so that row 3 - a zero row of A and a residual of 1.5 - bias - is exactly
    constant before the LayerNorm"""
    N, seed = 512, K * 7 + M
    g = sr.rng(seed)
    A, W, R = sr.values((M, K), dt, seed + 1, 0.7), sr.values((N, K), dt, seed + 2, 1.5 / math.sqrt(K)), sr.values((M, N), dt, seed + 3)
    bias = (np.round(0.3 * g.standard_normal(N) * 8) / 8).astype(f32)
    gamma, beta = (1.0 + 0.3 * g.standard_normal(N)).astype(f32), (0.2 * g.standard_normal(N)).astype(f32)
    if M > 3:
        A[0][3], A[1][3] = 0, 0
        R[0][3], R[1][3] = sr.split_rn((f32(1.5) - bias).astype(f32), dt)
        assert not R[1][3].any()
    return A, W, R, bias, gamma, beta


@DT
@pytest.mark.parametrize("K,M", GEMM_LN_CASES)
def test_gemm_residual_layernorm(K, M, dt):
    N, eps = 512, 1e-12
    A, W, R, bias, gamma, beta = gemm_ln_case(K, M, dt)
    lda, ldw, ldr, ldo = M + 7, N + 9, M + 5, M + 3
    At, a_ptr = panel_operand(A, dt, lda)
    Wt, w_ptr = panel_operand(W, dt, ldw)
    Rt, r_ptr = panel_operand(R, dt, ldr)
    bd, gd, btd = dev32(bias), dev32(gamma), dev32(beta)
    out = nans(2 * (N // 32) * ldo * 32, T16[dt])
    keys = sc.keys_of(lambda: check(lib().mh_split_gemm_res_ln(a_ptr, lda, w_ptr, ldw, bd.data_ptr(), r_ptr, ldr, gd.data_ptr(), btd.data_ptr(), eps,
                                                               out.data_ptr(), ldo, M, N, K, dt, current_stream()), "mh_split_gemm_res_ln"))
    assert keys == [sc.gemm_ln_key(sr.NAME[dt], K)], keys
    compare("ln-K%d-M%d" % (K, M), dt, "y", sr.val(read_panels(out, dt, M, N, ldo, "out")), sr.gemm_ln(A, W, bias, R, gamma, beta, eps, dt))


# ------------------------------------------------------------------------------------------------------------------ attention
ATTN_L = (8, 64, 72, 200, 248, 256, 264, 512)
PROFILES = ("plain", "rising", "falling")
# (dh, L, B, nh, profile, pitched: k_offset = H + 8, ld_qk = 2H + 16, ld_vt and ld_ctx larger than B L; scale factor on 1 / sqrt(dh))
ATTN_CASES = []
for _d, _dh in enumerate((16, 32, 64)):
    for _i, _L in enumerate(ATTN_L):
        # every (dh, waves, tail) class - L = 72 | 64 | 264 | 512 and their neighbours - gets all three profiles
        for _p in (PROFILES if _L in (64, 72, 264, 512) else (PROFILES[(_i + _d) % 3],)):
            _six = (_i + PROFILES.index(_p)) % 2
            ATTN_CASES.append((_dh, _L, 3 if _six else 1, 2 if _six or _dh == 16 else 1, _p, (_i + _d + PROFILES.index(_p)) % 2, 1.0))
    ATTN_CASES.append((_dh, 200, 1, 2, "underflow", 1, 250.0))
    ATTN_CASES.append((_dh, 512, 1, 2, "underflow", 0, 250.0))


def _attn_id(c):
    return "dh%d-L%d-B%d-nh%d-%s-%s%s" % (c[0], c[1], c[2], c[3], c[4], "pitched" if c[5] else "tight", "" if c[6] == 1.0 else "-x%g" % c[6])


@DT
@pytest.mark.parametrize("case", ATTN_CASES, ids=_attn_id)
def test_attention(case, dt):
    dh, L, B, nh, profile, pitched, factor = case
    H, Ntok = nh * dh, B * L
    scale = factor / math.sqrt(dh)
    q, k, v = sr.attn_inputs(B, L, nh, dh, profile, dt, seed=dh * 1000 + L + B)
    koff, ldq, ldv, ldc = (H + 8, 2 * H + 16, Ntok + 8, Ntok + 5) if pitched else (H, 2 * H, Ntok, Ntok)
    gap = 16 if pitched else 0          # NaN elements between the hi and lo parts
    qk_part, vt_part = Ntok * ldq + gap, H * ldv + gap
    qk = np.full((2, qk_part), np.nan, dtype=f32)
    vt = np.full((2, vt_part), np.nan, dtype=f32)
    for p in range(2):
        rows = qk[p, :Ntok * ldq].reshape(Ntok, ldq)
        rows[:, :H], rows[:, koff:koff + H] = q[p], k[p]
        vt[p, :H * ldv].reshape(H, ldv)[:, :Ntok] = v[p].T
    qd, vd = dev16(qk, dt), dev16(vt, dt)
    ctx = nans(2 * (H // 32) * ldc * 32, T16[dt])
    keys = sc.keys_of(lambda: check(lib().mh_split_attention(qd.data_ptr(), ldq, koff, qk_part, vd.data_ptr(), ldv, vt_part, ctx.data_ptr(), ldc, B, L, nh, dh,
                                                             scale, dt, current_stream()), "mh_split_attention"))
    assert keys == [sc.attn_key(sr.NAME[dt], dh, L)], keys
    ref = sr.attention(q, k, v, B, L, nh, dh, scale, dt)
    if profile == "underflow":          # (the case is about exp2 returning zero: all but a few keys of a row must be there)
        c = float(sr.scale_log2e(scale))
        s = np.einsum("bhid,bhjd->bhij", sr._heads(sr.val(q), B, L, nh, dh), sr._heads(sr.val(k), B, L, nh, dh)) * c
        assert np.median(((s - s.max(-1, keepdims=True)) < -150).mean(-1)) > 0.5
    compare(_attn_id(case), dt, "ctx", sr.val(read_panels(ctx, dt, Ntok, H, ldc, "ctx")), ref)
