"""The tolerance tests/test_train_layer_matrix_gpu.py holds mh_train_layer_bwd to (tests/layer_ref.py: the kernels' e_rms / e_max within
2x / 3x of a float64 emulation's own, per output tensor) is neither too tight nor blind: a second realisation of the same roundings - every
fp32 sum taken in float32 - stays inside it, and every wiring error of layer_ref.MUTANTS falls outside it on at least one tensor.  No
device and no kernel: the forward's saved tensors are layer_ref.forward_saved.  Plus the host-only queries of csrc/train_layer.hip.

Measured here (python -m pytest tests/test_train_layer_bound_cpu.py -s prints every line; recorded in profiles/train_layer_matrix.txt):
the second realisation's worst share of the margin is 0.50 (e_rms) / 0.34 (e_max) - the bf16 roundings dominate and fall the same way in
both, so its errors equal the emulation's to three digits everywhere but in dln2, which no bf16 rounding precedes; the mutants exceed the
margin by 13x ((b), 1 / (1 - p) missing at p = 0.1) to over 1e6x ((h)); none is weakly seen."""
import functools
import math

import pytest
import torch

import attention_ref as ar
import layer_ref as lr

from musediffusion_amd._lib import lib

# (B, L, heads, F, p = (attn, ao, ffn))
CASES = {"p0": (1, 512, 8, 256, (0.0, 0.0, 0.0)), "drop": (1, 576, 16, 256, (0.1, 0.1, 0.1))}


@functools.lru_cache(maxsize=None)
def setup(name):
    """(saved, weights, masks, dy, heads, reference backward, errors of the emulation) of a case - computed once, never modified"""
    B, L, nh, F, p = CASES[name]
    w = lr.layer_inputs(B, L, F)
    masks = lr.random_masks(B, L, nh, p, seed=3) if any(p) else lr.no_masks()
    saved = lr.forward_saved(w, masks, nh, B, L)
    ref = lr.backward(saved, w, masks, w["dy"], nh)
    emu = lr.errors(lr.backward_emulated(saved, w, masks, w["dy"], nh), ref)
    return saved, w, masks, w["dy"], nh, ref, emu


@pytest.mark.parametrize("name", list(CASES))
def test_a_second_realisation_stays_inside_the_margins(name):
    saved, w, masks, dy, nh, ref, emu = setup(name)
    second = lr.errors(lr.backward_emulated(saved, w, masks, dy, nh, f32=True), ref)
    print()
    print("\n".join(lr.table(name, second, emu, label="float32 sums")))
    for n, (rms, mx) in emu.items():
        assert 0 < rms < 0.05 and 0 < mx < 0.05, "%s: the emulation itself is off (%g, %g)" % (n, rms, mx)
    m = lr.margins(second, emu)
    bad = {n: v for n, v in m.items() if max(v) > 1.0}
    assert not bad, "a correct implementation falls outside the margins: %s" % bad


@pytest.mark.parametrize("mutant", list(lr.MUTANTS))
def test_every_mutant_falls_outside_the_margins(mutant):
    what, needs_drop, needs_split = lr.MUTANTS[mutant]
    seen = []
    for name in (["drop"] if needs_drop else list(CASES)):
        saved, w, masks, dy, nh, ref, emu = setup(name)
        got = lr.errors(lr.backward_emulated(saved, w, masks, dy, nh, mutant=mutant, splits=2), ref)
        factor, tensor = lr.worst(lr.margins(got, emu))
        seen.append(factor)
        print("\nLAYER-MUTANT (%s) %-62s case %-4s exceeds the margin %.3gx on %s%s"
              % (mutant, what, name, factor, tensor, "  [weakly seen]" if 1.0 < factor < 2.0 else ""))
    assert max(seen) > 1.0, "mutant (%s) %s: inside the margins (%s)" % (mutant, what, seen)


def test_given_the_references_own_forward_the_attention_emulation_is_attention_ref_emulate():
    """layer_ref.attention_bwd_emulated restates attention_ref.emulate's backward only to take O and lse2 as arguments"""
    B, nh, L, dh = 1, 2, 512, 32
    _, _, q, k, v, dO = ar.stress_inputs(B, nh, L, dh, seed=5)
    keep = torch.rand(B * nh, L, L, generator=torch.Generator().manual_seed(6)) >= 0.1
    scale = 1.0 / math.sqrt(dh)
    for kp, p in ((None, 0.0), (keep, 0.1)):
        r = ar._reference(q.double(), k.double(), v.double(), scale, kp, p, None)
        want = ar.emulate(q, k, v, scale, kp, p, dO)
        got = lr.attention_bwd_emulated(q, k, v, scale, kp, p, dO, r["o_given"], r["lse2_given"])
        for n in ("dq", "dk", "dv"):
            assert torch.equal(got[n], want[n]), n


def test_split_rows_cover_the_tokens_in_slices_that_differ_by_one_step():
    for N, S in ((1664, 3), (1152, 2), (512, 1), (2080, 5)):
        rows = lr.split_rows(N, S)
        assert rows[0][0] == 0 and rows[-1][1] == N and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
        steps = [(b - a) // 32 for a, b in rows]
        assert max(steps) - min(steps) <= 1 and min(steps) >= 1
    assert len({b - a for a, b in lr.split_rows(1664, 3)}) == 2          # 52 K-steps in 3 slices: unequal


# ------------------------------------------------------------------------------------------------------------------ host-only queries
SUPPORTED = [
    # B, L, H, F, nh, served
    (1, 512, 512, 256, 8, 1), (2, 576, 512, 2048, 16, 1), (2, 832, 512, 1024, 8, 1),
    (1, 512, 768, 256, 12, 0), (1, 512, 256, 256, 4, 0),          # H other than 512
    (1, 512, 512, 384, 8, 0), (1, 512, 512, 0, 8, 0),            # F % 256
    (1, 544, 512, 256, 8, 0),                                    # L % 64
    (1, 448, 512, 256, 8, 0), (4, 256, 512, 256, 8, 0),          # L < 512
    (1, 512, 512, 256, 32, 0), (1, 512, 512, 256, 4, 0),         # head dim 16, 128
    (1, 512, 512, 256, 7, 0), (1, 512, 512, 256, 0, 0),          # H % nh, no heads
    (0, 512, 512, 256, 8, 0),
]


@pytest.mark.parametrize("B,L,H,F,nh,served", SUPPORTED)
def test_supported_truth_table_and_scratch_bytes(B, L, H, F, nh, served):
    L_ = lib()
    assert int(L_.mh_train_layer_supported(B, L, H, F, nh)) == served
    N = B * L
    if served:
        a, b = int(L_.mh_train_layer_scratch_bytes(B, L, H, F, nh, N)), int(L_.mh_train_layer_scratch_bytes(B, L, H, F, nh, N + 64))
        assert 0 < a < b and a % 256 == 0 and b % 256 == 0
        # the panel buffers m, d1 and dqkv grow with ld: 64 more rows of H + F + 3 H bf16 columns
        assert b - a == 64 * (H + F + 3 * H) * 2
        assert int(L_.mh_train_layer_scratch_bytes(B, L, H, F, nh, N - 1)) == 0          # ld < B L
        assert int(L_.mh_train_layer_scratch_bytes(B, L, H, F, nh, 0)) == 0
    else:
        assert int(L_.mh_train_layer_scratch_bytes(B, L, H, F, nh, max(N, 512) + 64)) == 0


@pytest.mark.parametrize("F", [256, 1024, 2048])
def test_grad_floats_is_the_sum_of_the_twelve_blocks(F):
    H = lr.H
    sizes = [3 * H * H, 3 * H, H * H, H, F * H, F, H * F, H, H, H, H, H]          # training._EncoderLayer.backward's split
    assert lr.grad_sizes(F) == sizes
    assert int(lib().mh_train_layer_grad_floats(H, F)) == sum(sizes)
    import inspect

    from musediffusion_amd import training
    assert "sizes = [3 * H * H, 3 * H, H * H, H, F * H, F, H * F, H, H, H, H, H]" in inspect.getsource(training._EncoderLayer.backward)
