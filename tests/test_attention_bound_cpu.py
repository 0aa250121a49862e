"""The attention parity matrix's reference passes its own tolerance (CPU): a float64 emulation that rounds exactly where the streaming
kernels round (tests/attention_ref.py: emulate - fp32 softmax sum and lse2, P and dS to bf16 before the second product, D from the bf16 O,
outputs to their storage types) stays inside the per-element bounds of `reference` at the matrix' shape kinds, on its stress inputs
(dominant keys, a (batch, head) with every score far below zero).  What the emulation does not contain - the hardware exp2, the online
rescale, the accumulation order - is what tests/test_attention_matrix_gpu.py measures on the kernels."""
import math

import pytest
import torch

import attention_ref as ar

OUTPUTS = ("ctx", "lse2", "D", "dq", "dk", "dv")


@pytest.mark.parametrize("L,dh,p", [(512, 64, 0.0), (528, 32, 0.0), (1024, 64, 0.1), (784, 32, 0.1)])
def test_emulated_kernel_rounding_stays_within_the_bounds(L, dh, p):
    n = 3
    _, _, q, k, v, dO = ar.stress_inputs(1, n, L, dh, seed=L + dh, hot=(2,))
    keep = (torch.rand(n, L, L, generator=torch.Generator().manual_seed(L)) >= p) if p else None
    scale = 1.0 / math.sqrt(dh)
    ref = ar.reference(q, k, v, scale, keep, p, dO)
    worst = ar.ratios(ar.emulate(q, k, v, scale, keep, p, dO), ref, OUTPUTS)
    print("L=%d dh=%d p=%g worst err / bound: %s; median ctx atol %.2e, median dQ atol / max |dQ| %.2e"
          % (L, dh, p, " ".join("%s %.2f" % kv for kv in worst.items()), float(ref["ctx_atol"].median()),
             float(ref["dq_atol"].median() / ref["dq"].abs().max())))
    assert all(w <= 1.0 for w in worst.values()), worst
    if p:      # the bounds see a 1 / (1 - p) that is missing from one output
        em = ar.emulate(q, k, v, scale, keep, p, dO)
        em["dq"] = em["dq"] * (1.0 - p)
        assert ar.ratios(em, ref, ("dq",))["dq"] > 1.0


def test_prescaled_queries_within_the_bounds():
    """the pre-scaled form's reference: softmax of ln 2 x (stored q) k^T on the queries as stored (scale x log2(e) folded in, rounded again)"""
    _, _, q, k, v, _ = ar.stress_inputs(1, 3, 512, 64, seed=3, pre=True)
    ref = ar.reference(q, k, v, math.log(2.0))
    worst = ar.ratios(ar.emulate(q, k, v, math.log(2.0)), ref, ("ctx", "lse2"))
    assert all(w <= 1.0 for w in worst.values()), worst
    # ... and it is the same attention, up to the second rounding of q, as the plain form's on the unscaled queries
    _, _, q0, k0, v0, _ = ar.stress_inputs(1, 3, 512, 64, seed=3)
    plain = ar.reference(q0, k0, v0, 0.125)
    assert torch.equal(k0, k) and float((plain["ctx"] - ref["ctx"]).abs().max()) < 0.05
