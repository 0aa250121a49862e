"""mh_train_layer_fwd / mh_train_layer_bwd (csrc/train_layer.hip: one HF BertLayer of the bf16 training step, forward and backward, as
about 25 launches over K32-panel buffers) against the float64 layer reference of tests/layer_ref.py, through the C ABI (_lib.TrainLayer),
at the smallest shapes at which each path of the wiring exists.  The kernels have their own parity matrices; this one checks what picks
buffers, dropout sites, residual branches, gradient offsets, split counts and the side stream.

Every output buffer, `grads`, `dx` and the backward's scratch start as NaN, and so do rows N .. ld - 1 of every panel buffer, the caller's
x included (training.py allocates them uninitialised): after each call every result element is finite and the pad rows are still NaN.

* forward: every buffer the forward leaves behind against layer_ref.forward_stages - the float64 value of that ONE stage from the stage's
  stored inputs, element by element, with the bound of the kernel's own matrix (nothing new);
* backward: dx and the twelve blocks of `grads` against layer_ref.backward, held to the error of layer_ref.backward_emulated on the same
  saved tensors: e_rms <= 2 e_rms(emulated) + 2^-22 and e_max <= 3 e_max(emulated) + 2^-22 per tensor (tests/test_train_layer_bound_cpu.py:
  a second realisation stays inside, every wiring mutant falls outside).

Which case covers what (H = 512 throughout; the split counts are asserted through mh_gemm_dw_splits, so a change of that rule fails
here instead of dropping coverage):

    N = 512, all four mh_gemm_dw_splits == 1 (dw() writes straight into grads)   n512-off, n512-dh32-f2048-philox, n512-dh64-philox
    splits == 2 (and seq_len 576: the streaming attention ends in a partial 256-key stage)   s2-attn-injected, s2-ao-philox, s2-ffn-injected
    splits == 3 with unequal slices (B 2, L 832: 52 K-steps = 17 + 17 + 18)      s3-injected
    head dim 64 (8 heads)                 n512-off, n512-dh64-philox, s2-attn-injected, s2-ffn-injected, s3-injected
    head dim 32 (16 heads)                n512-dh32-f2048-philox, s2-ao-philox
    F = 256 / 1024 / 2048 (> 3 H)         n512-off and others / s2-attn-injected / n512-dh32-f2048-philox
    ld = N                                n512-off, s2-ao-philox
    ld = N + 64                           every other case
    y_panel 0 / 1                         n512-off, s2-ao-philox, s2-ffn-injected / the others; the same y bit for bit: test_options_...
    dropout off                           n512-off
    all three sites, p = 0.1 / 0.2 / 0.05, different offsets      n512-dh32-f2048-philox (Philox), s3-injected (injected)
    each site alone                       s2-attn-injected, s2-ao-philox, s2-ffn-injected
    Philox masks (bits_in = 0; dense masks restated by dense_keep, keep bits decoded from what the forward wrote)
                                          n512-dh32-f2048-philox, n512-dh64-philox, s2-ao-philox
    injected masks (mh_dropout.mask bytes; bits_in = 1 with mask_to_bits)        s2-attn-injected, s2-ffn-injected, s3-injected
    side_stream NULL / == stream / a second stream     per case (column `side`); bit-identical dx and grads, read on the caller's stream
                                          without a device-wide synchronise: test_options_are_bit_identical
    the same call twice                   test_options_are_bit_identical
    argument checks                       test_forward_argument_errors / test_backward_argument_errors

Measured on an MI355X (256 CUs): profiles/train_layer_matrix.txt."""
import ctypes as C
import functools

import pytest
import torch

import gemm_census as gc
import layer_ref as lr

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import MH_ERR_INVALID, lib  # noqa: E402
from test_dropout_gpu import bits_to_mask, mask_to_bits  # noqa: E402
from test_gemm_matrix_gpu import DEV, close  # noqa: E402
from test_round6_train_gpu import to_panel  # noqa: E402

NAN = float("nan")
H = lr.H
BF, F32 = torch.bfloat16, torch.float32
P3 = (0.1, 0.2, 0.05)

# id: (B, L, heads, F, pad rows, y_panel, p = (attn, ao, ffn), injected masks, side stream, expected splits)
CASES = {
    "n512-off": (1, 512, 8, 256, 0, 0, (0.0, 0.0, 0.0), False, "null", 1),
    "n512-dh32-f2048-philox": (1, 512, 16, 2048, 64, 1, P3, False, "other", 1),
    "n512-dh64-philox": (1, 512, 8, 256, 64, 1, (0.1, 0.1, 0.1), False, "same", 1),
    "s2-attn-injected": (2, 576, 8, 1024, 64, 1, (0.1, 0.0, 0.0), True, "same", 2),
    "s2-ao-philox": (2, 576, 16, 256, 0, 0, (0.0, 0.2, 0.0), False, "other", 2),
    "s2-ffn-injected": (2, 576, 8, 256, 64, 0, (0.0, 0.0, 0.05), True, "null", 2),
    "s3-injected": (2, 832, 8, 256, 64, 1, P3, True, "other", 3),
}
SITES = ("attn", "ao", "ffn")


@functools.lru_cache(maxsize=2)
def device_weights(B, L, F):
    """the layer's operands on the device: weight panels and their transposes built on the host, vectors fp32"""
    w = lr.layer_inputs(B, L, F)
    d = {}
    for name, key in (("wqkv", "Wqkv"), ("wao", "Wao"), ("w1", "W1"), ("w2", "W2")):
        d[name], d[name + "_t"] = to_panel(w[key]), to_panel(w[key].T.contiguous())
    for name in ("bqkv", "bao", "b1", "b2", "ln1_g", "ln1_b", "ln2_g", "ln2_b"):
        d[name] = w[name].float().contiguous().to(DEV)
    return d


def panel_nan(cols, ld):
    return torch.full((cols // 32, ld, 32), NAN, dtype=BF, device=DEV)


def read_panel(buf, N, name):
    """panels [cols / 32][ld][32] -> [N, cols] on the host; rows N .. ld - 1 must still be NaN"""
    b = buf.cpu()
    assert bool(torch.isnan(b[:, N:].float()).all()), "%s: rows behind the B L tokens were written" % name
    return b[:, :N].permute(1, 0, 2).reshape(N, -1)


class Layer:
    """the buffers and the descriptor of one case; every output starts as NaN"""

    def __init__(self, B, L, nh, F, pad, y_panel, p, injected, mask_seed=11):
        self.B, self.L, self.nh, self.F, self.N, self.ld, self.y_panel = B, L, nh, F, B * L, B * L + pad, y_panel
        N, ld = self.N, self.ld
        self.w = lr.layer_inputs(B, L, F)
        self.dw = device_weights(B, L, F)
        t = self.t = _lib.TrainLayer()
        t.B, t.L, t.H, t.F, t.nh, t.ln_eps, t.ld = B, L, H, F, nh, lr.LN_EPS, ld
        for name, v in self.dw.items():
            setattr(t, name, v.data_ptr())
        # dropout sites: three different offsets; injected: the keep flags come from the host
        self.p, self.injected = tuple(float(v) for v in p), injected
        self.masks = lr.random_masks(B, L, nh, p, mask_seed) if injected else None
        self.descs, self.keep_alive = {}, []
        for i, s in enumerate(SITES):
            d = _lib.Dropout()
            d.p, d.seed, d.offset, d.mask = self.p[i], 0x5DEECE66D ^ (17 + i), ((3 + i) << 16) | (5 * i + 1), None
            if injected and self.p[i] > 0 and s != "attn":
                m = self.masks[s][0].to(torch.uint8).contiguous().to(DEV)
                self.keep_alive.append(m)
                d.mask = m.data_ptr()
            self.descs[s] = d
            setattr(t, "drop_" + s, d)
        self.bits = None
        if self.p[0] > 0:
            words = int(lib().mh_dropout_bits_words(B * nh, L))
            self.bits = mask_to_bits(self.masks["attn"][0].to(DEV)) if injected else torch.zeros(words, dtype=torch.int32, device=DEV)
            assert self.bits.numel() == words
            t.keep_bits, t.bits_in = self.bits.data_ptr(), int(injected)
        # the caller's x: panels, the rows behind N poisoned
        self.x = panel_nan(H, ld)
        self.x[:, :N] = self.w["x"].reshape(N, H // 32, 32).permute(1, 0, 2).to(DEV)
        self.dy = self.w["dy"].contiguous().to(DEV)
        t.x, t.dy, t.y_panel = self.x.data_ptr(), self.dy.data_ptr(), y_panel
        self.fwd_bufs = {}
        self.fill_forward()
        self.scratch_bytes = int(lib().mh_train_layer_scratch_bytes(B, L, H, F, nh, ld))
        assert self.scratch_bytes > 0
        self.fill_backward()

    def fill_forward(self):
        N, ld, F, t = self.N, self.ld, self.F, self.t
        full = lambda *s, dt=BF: torch.full(s, NAN, dtype=dt, device=DEV)  # noqa: E731
        b = self.fwd_bufs = {"qkv": full(N, 3 * H), "vt": full(N * H + 256), "ctx": panel_nan(H, ld), "lse": full(self.B * self.nh * self.L, dt=F32),
                             "pre1": full(N, H), "x1": panel_nan(H, ld), "g": panel_nan(F, ld), "dact": panel_nan(F, ld), "pre2": full(N, H),
                             "y": panel_nan(H, ld) if self.y_panel else full(N, H)}
        for name, buf in b.items():
            setattr(t, name, buf.data_ptr())

    def fill_backward(self):
        t = self.t
        self.dx = torch.full((self.N, H), NAN, dtype=BF, device=DEV)
        self.grads = torch.full((sum(lr.grad_sizes(self.F)),), NAN, dtype=F32, device=DEV)
        self.scratch = torch.full((self.scratch_bytes,), 255, dtype=torch.uint8, device=DEV)          # (0xFFFF / 0xFFFFFFFF: NaN as bf16 and as fp32)
        t.dx, t.grads, t.scratch, t.scratch_bytes = self.dx.data_ptr(), self.grads.data_ptr(), self.scratch.data_ptr(), self.scratch_bytes

    def forward(self, stream=None):
        return int(lib().mh_train_layer_fwd(C.byref(self.t), stream if stream is not None else _lib.current_stream()))

    def backward(self, side=None, stream=None):
        self.t.side_stream = side
        return int(lib().mh_train_layer_bwd(C.byref(self.t), stream if stream is not None else _lib.current_stream()))

    def saved(self):
        """the forward's buffers on the host, token-major; panel pad rows checked"""
        N, b = self.N, self.fwd_bufs
        s = {"x": self.w["x"]}
        for name, buf in b.items():
            if name in ("ctx", "x1", "g", "dact") or (name == "y" and self.y_panel):
                s[name] = read_panel(buf, N, name)
            elif name == "lse":
                s[name] = buf.cpu().view(self.B * self.nh, self.L)
            else:
                s[name] = buf.cpu()
        assert bool(torch.isnan(self.x[:, N:].float()).all())
        return s

    def host_masks(self):
        """the keep flags of the three sites as the kernels drew (Philox) or were given them"""
        if self.injected:
            return self.masks
        out = {}
        for i, s in enumerate(SITES):
            d, p = self.descs[s], float(torch.tensor(self.p[i], dtype=F32))
            if self.p[i] == 0:
                out[s] = (None, 0.0)
            elif s == "attn":
                out[s] = (bits_to_mask(self.bits, self.B * self.nh, self.L).cpu(), p)
            else:
                out[s] = (torch.from_numpy(gc.dense_keep(self.N, H, self.p[i], d.seed, d.offset)), p)
        return out

    def results(self):
        g = self.grads.cpu()
        out = dict(zip(lr.GRAD_NAMES, g.split(lr.grad_sizes(self.F))))
        out["dx"] = self.dx.cpu()
        return out


def split_counts(N, F):
    return [int(lib().mh_gemm_dw_splits(N, m, n)) for m, n in ((H, F), (F, H), (H, H), (3 * H, H))]


@pytest.mark.parametrize("case", list(CASES))
def test_layer_against_the_float64_reference(case):
    B, L, nh, F, pad, y_panel, p, injected, side, splits = CASES[case]
    ly = Layer(B, L, nh, F, pad, y_panel, p, injected)
    N = ly.N
    got_splits = split_counts(N, F)
    assert got_splits == [splits] * 4, "mh_gemm_dw_splits changed: this case no longer covers splits == %d (%s)" % (splits, got_splits)
    if splits == 3:
        assert len({b - a for a, b in lr.split_rows(N, 3)}) == 2          # unequal slices
    print("\nLAYER-CASE %s B %d L %d heads %d F %d ld N+%d y_panel %d p %s %s side %s splits %s"
          % (case, B, L, nh, F, pad, y_panel, p, "injected" if injected else "philox", side, got_splits))
    # ---- forward
    _lib.check(ly.forward(), "mh_train_layer_fwd")
    torch.cuda.synchronize()
    saved = ly.saved()
    masks = ly.host_masks()
    stages = lr.forward_stages(saved, ly.w, masks, nh)
    for name in lr.FORWARD_BUFFERS:
        ref, atol, rtol = stages[name]
        got = saved[name].double().reshape(ref.shape)
        assert bool(torch.isfinite(got).all()), "%s: not finite / never written" % name
        if name == "vt":
            assert torch.equal(got, ref), "vt is not head_permute mode 4 of the stored V"
            continue
        print("LAYER-FWD %-22s %-5s worst err / bound %.3f" % (case, name, float(((got - ref).abs() / (atol + rtol * ref.abs())).max())))
        close("%s: %s" % (case, name), got, ref, atol, rtol)
    # ---- backward
    other = torch.cuda.Stream()
    side_ptr = {"null": None, "same": _lib.current_stream(), "other": other.cuda_stream}[side]
    _lib.check(ly.backward(side_ptr), "mh_train_layer_bwd")
    torch.cuda.synchronize()
    res = ly.results()
    for name, v in res.items():
        assert bool(torch.isfinite(v.float()).all()), "%s: %d elements not finite / never written" % (name, int((~torch.isfinite(v.float())).sum()))
    ref = lr.backward(saved, ly.w, masks, ly.w["dy"], nh)
    e_emu = lr.errors(lr.backward_emulated(saved, ly.w, masks, ly.w["dy"], nh), ref)
    e_got = lr.errors(res, ref)
    print("\n".join(lr.table(case, e_got, e_emu)))
    bad = {n: v for n, v in lr.margins(e_got, e_emu).items() if max(v) > 1.0}
    assert not bad, "%s: outside e_rms <= 2 e_rms(emulated) + 2^-22, e_max <= 3 e_max(emulated) + 2^-22 (shares of the margin): %s" % (case, bad)


def test_options_are_bit_identical():
    """y_panel 0 / 1 store the same y; side_stream NULL / == stream / a second stream, and the same call twice, give the same dx and
    grads bit for bit - read on the caller's (non-default) stream without a device-wide synchronise, after the NaN prefill"""
    B, L, nh, F, pad = 2, 576, 8, 256, 64
    assert split_counts(B * L, F) == [2] * 4          # (the folds this test moves between streams exist)
    ly = Layer(B, L, nh, F, pad, 1, P3, False)
    _lib.check(ly.forward(), "mh_train_layer_fwd")
    torch.cuda.synchronize()
    first = ly.saved()
    bits = ly.bits.clone()
    for y_panel in (1, 0):
        ly.y_panel = ly.t.y_panel = y_panel
        ly.fill_forward()
        _lib.check(ly.forward(), "mh_train_layer_fwd")
        torch.cuda.synchronize()
        again = ly.saved()
        for name in lr.FORWARD_BUFFERS:
            assert torch.equal(first[name].view(torch.int16 if first[name].dtype == BF else torch.int32),
                               again[name].view(torch.int16 if again[name].dtype == BF else torch.int32)), "y_panel %d: %s differs" % (y_panel, name)
        assert torch.equal(bits, ly.bits)
    main, other = torch.cuda.Stream(), torch.cuda.Stream()
    main.wait_stream(torch.cuda.current_stream())
    outs, held = [], []
    with torch.cuda.stream(main):
        for side in (None, main.cuda_stream, other.cuda_stream, other.cuda_stream):
            held.append((ly.dx, ly.grads, ly.scratch))
            ly.fill_backward()
            _lib.check(ly.backward(side, stream=main.cuda_stream), "mh_train_layer_bwd")
            outs.append((ly.dx.cpu(), ly.grads.cpu()))          # (a copy on `main` and a wait for `main` alone)
    torch.cuda.synchronize()
    dx0, g0 = outs[0]
    assert bool(torch.isfinite(dx0.float()).all()) and bool(torch.isfinite(g0).all())
    for what, (dx, g) in zip(("side == stream", "a second stream", "a second stream, again"), outs[1:]):
        assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16)), "dx differs: %s" % what
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32)), "grads differ: %s" % what


# ------------------------------------------------------------------------------------------------------------------ argument checks
def _rejected(rc, what):
    assert rc == MH_ERR_INVALID, "%s: returned %d, not MH_ERR_INVALID" % (what, rc)
    msg = lib().mh_last_error()
    assert msg and b"train_layer" in msg, "%s: no message (%r)" % (what, msg)


def _all_nan(bufs, what):
    for name, b in bufs.items():
        v = b.view(BF) if b.dtype == torch.uint8 else b
        assert bool(torch.isnan(v.float()).all()), "%s: %s was written by a call that returned an error" % (what, name)


def _error_layer():
    return Layer(1, 512, 8, 256, 64, 1, (0.0, 0.0, 0.0), False)


FWD_ERRORS = {
    "unsupported shape (L % 64)": lambda ly: setattr(ly.t, "L", 544),
    "unsupported shape (head dim 128)": lambda ly: setattr(ly.t, "nh", 4),
    "null activation buffer": lambda ly: setattr(ly.t, "ctx", None),
    "drop_attn active with keep_bits NULL": lambda ly: (setattr(ly.t.drop_attn, "p", 0.1), setattr(ly.t, "keep_bits", None)),
    "ld < N": lambda ly: setattr(ly.t, "ld", ly.N - 32),
}
BWD_ERRORS = dict(FWD_ERRORS)
BWD_ERRORS["scratch_bytes one byte short"] = lambda ly: setattr(ly.t, "scratch_bytes", ly.scratch_bytes - 1)
BWD_ERRORS["null dx"] = lambda ly: setattr(ly.t, "dx", None)


@pytest.mark.parametrize("what", list(FWD_ERRORS))
def test_forward_argument_errors(what):
    """plain argument checks that return before any launch: MH_ERR_INVALID, a message, every NaN-prefilled output untouched"""
    ly = _error_layer()
    FWD_ERRORS[what](ly)
    _rejected(ly.forward(), what)
    torch.cuda.synchronize()
    _all_nan(ly.fwd_bufs, what)


@pytest.mark.parametrize("what", list(BWD_ERRORS))
def test_backward_argument_errors(what):
    ly = _error_layer()
    BWD_ERRORS[what](ly)
    _rejected(ly.backward(), what)
    torch.cuda.synchronize()
    _all_nan({"dx": ly.dx, "grads": ly.grads, "scratch": ly.scratch}, what)
