"""Launch census: every GEMM-family kernel variant the product launches at the bench.py shapes must be checked against a reference by
some test.  The census records eager runs of the sampler's forward (every compute mode), one reverse step with the rounding, training
micro-steps (panel-layer tape and the op-per-node tape) with the library's per-launch recorder (mh_profile_start / mh_profile_stop), turns
each GEMM-family launch into a key (tests/gemm_census.py: census_key) and looks it up in PARITY.  A new variant, or a production shape that
the dispatcher sends somewhere new, fails here until a parity case reaches it.

PARITY maps each key to the tests that compare that variant with a reference: `module::test[id]` for one case, `module::test` for all of
a test's cases."""
import os
import subprocess
import sys

import pytest

import gemm_census as gc

M = "tests/test_gemm_matrix_gpu.py::"
DENSE = M + "test_dense_variant_against_reference[%s]"
CLASSES = ("ragged", "multitile", "window")


def _defer(form):
    return [M + "test_deferred_layernorm_variant_against_reference[%s-%s]" % (form, c) for c in CLASSES]


def _qkv(form):
    return [M + "test_qkv_projection_against_reference[%s-%s]" % (form, c) for c in CLASSES]


def _dense(name, classes=("ragged", "multitile")):
    return [DENSE % ("%s-%s" % (name, c)) for c in classes]


PARITY = {
    # EPI 0 on the 256 x 128 / 256 x 256 tiles, the epilogue's form fixed at compile time (bit 16384: stage DMA as buffer loads)
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (1 << 16)> | tile=256x128": _dense("form1-rows") + [M + "test_gemm_batched_against_reference"],
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (1 << 16) | 16384> | tile=256x128": _dense("form1-panels", ("ragged", "multitile", "window")),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (1 << 16)> | tile=256x256": _dense("form1-rows-wide"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (2 << 16)> | tile=256x128": _dense("form2-rows"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (2 << 16) | 16384> | tile=256x128": _dense("form2-panels", ("ragged", "multitile", "window")),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (4 << 16)> | tile=256x128": _dense("form4-rows"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (4 << 16) | 16384> | tile=256x128": _dense("form4-panels", ("ragged", "multitile", "window")),
    "gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, (8 << 16)> | tile=256x128": _dense("form8-rows"),
    "gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, (8 << 16) | 16384> | tile=256x128": _dense("form8-panels", ("ragged", "multitile", "window")),
    # EPI 0, generic epilogue
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (0)> | tile=256x128": _dense("generic-f32out") + [M + "test_gemm_batched_against_reference"],
    "gemm_big_kernel<C, 0, MH_ACT_TANH, (0)> | tile=256x256": _dense("generic-tanh-pre-wide"),
    "gemm_big_kernel<C, 0, MH_ACT_SILU> | tile=256x128": _dense("silu"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, 64> | tile=256x128": _dense("dropout-res-rows"),
    # EPI 0 with deferred LayerNorm operands (DBG bits 128 A rows raw, 256 residual rows raw, 512 output statistics, 768 both)
    "gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, (128) | 16384> | tile=256x128": _defer("a-gelu"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (256) | 16384> | tile=256x128": _defer("r"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (512) | 16384> | tile=256x128": _defer("o"),
    "gemm_big_kernel<C, 0, MH_ACT_NONE, (768) | 16384> | tile=256x128": _defer("r-o"),
    # EPI 1: QKV projection with the head scatter
    "gemm_big_kernel<C, 1, MH_ACT_NONE, (32) | 16384> | tile=256x128": _qkv("plain"),
    "gemm_big_kernel<C, 1, MH_ACT_NONE, (128) | 16384> | tile=256x128": _qkv("defer-a"),
    # EPI 3: full-row LayerNorm epilogue (sampler; training with dropout and the pre-LayerNorm rows)
    "gemm_big_kernel<C, 3, MH_ACT_NONE, (0) | 16384> | tile=128x512pp": [
        M + "test_res_ln_full_row_tile_against_reference[%s]" % c for c in ("ragged-1000-96", "multitile-None-96", "window-520-160")],
    "gemm_big_kernel<C, 3, MH_ACT_NONE, (64) | 16384> | tile=128x512pp": _dense("ln-dropout", ("ragged", "multitile", "window")) +
    [DENSE % "ln-nodrop-train-ragged"],
    # the column-strip kernel (sampler FFN1): M a multiple of 256, K = 512 only - no ragged shape reaches it
    "gemm_strip_kernel<16, MH_ACT_GELU_ERF> | tile=256x128": _dense("strip", ("multitile", "multitile-bands", "window")),
    # fp32 parity mode: the 128 x 128 kernel (grid = tiles)
    "gemm_kernel<float, EPI> | tile=128x128 epi=0 dtype=0": [M + "test_f32_gemm_against_reference"],
    "gemm_kernel<float, EPI> | tile=128x128 epi=1 dtype=0": ["tests/test_kernels_gpu.py::test_gemm_qkv_layout"],
    # weight gradients
    "gemm_tn_kernel<2> | tile=256x128": [M + "test_weight_gradient_against_reference[1056-136-128-0-gemm_tn_kernel<2> | tile=256x128]"],
    "gemm_tn_kernel<8, 4> | tile=256x256": [M + "test_weight_gradient_against_reference[4128-392-512-0-gemm_tn_kernel<8, 4> | tile=256x256]"],
    "gemm_tn_kernel<8, 4, true> | tile=256x256": [
        M + "test_weight_gradient_against_reference[2080-544-512-1-gemm_tn_kernel<8, 4, true> | tile=256x256]"],
    # split precision (bf16x3 / f16x3)
    "split_gemm_kernel<T, MH_ACT_NONE> | tile=256x128 out=1": [
        M + "test_split_gemm_against_reference[%s-%s]" % (c, dt) for c in ("0-1-False-ragged", "0-1-True-multitile") for dt in ("bf16x3", "f16x3")],
    "split_gemm_kernel<T, MH_ACT_NONE> | tile=256x128 out=2": [
        M + "test_split_gemm_against_reference[%s-%s]" % (c, dt) for c in ("0-2-False-ragged", "0-2-False-multitile") for dt in ("bf16x3", "f16x3")],
    "split_gemm_kernel<T, MH_ACT_TANH> | tile=256x128 out=0": [
        M + "test_split_gemm_against_reference[%s-%s]" % (c, dt) for c in ("1-0-False-ragged", "1-0-False-multitile") for dt in ("bf16x3", "f16x3")],
    "split_gemm_kernel<T, MH_ACT_GELU_ERF> | tile=256x128 out=0": [
        M + "test_split_gemm_against_reference[%s-%s]" % (c, dt) for c in ("2-0-False-ragged", "2-0-True-multitile") for dt in ("bf16x3", "f16x3")],
    "split_gemm_ln_kernel<T> | tile=128x512": [M + "test_split_gemm_res_ln_against_reference"],
}


@pytest.mark.gpu
def test_every_launched_gemm_variant_has_a_parity_test():
    import torch
    dev = torch.device("cuda", 0)
    seen = {}
    for name, run in gc.WORKLOADS.items():
        recs = run(dev)
        # (an empty record would make the census pass vacuously: launches that bypass the recorder, a graph replay)
        assert recs, "workload %r recorded no GEMM-family launch" % name
        for key, note in recs:
            seen.setdefault(key, [0, set(), note])
            seen[key][0] += 1
            seen[key][1].add(name)
        torch.cuda.empty_cache()
    print("\n%-78s %6s  %s" % ("GEMM variant launched (census key)", "calls", "parity tests / workloads"))
    for key in sorted(seen):
        n, names, note = seen[key]
        print("%-78s %6d  %s" % (key, n, "%d test(s)" % len(PARITY[key]) if key in PARITY else "NONE"))
        print("%-78s %6s  %s | e.g. %s" % ("", "", ", ".join(sorted(names)), note))
    missing = sorted(k for k in seen if k not in PARITY)
    assert not missing, "launched by the product, covered by no parity test:\n  " + "\n  ".join(missing)


def test_parity_table_names_existing_tests():
    """every test PARITY names is collected (pytest --collect-only over the modules it names; nothing runs)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ids = sorted({t for tests in PARITY.values() for t in tests})
    modules = sorted({t.split("::")[0] for t in ids})
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", "-m", "gpu or not gpu", *modules],
                       cwd=repo, capture_output=True, text=True, timeout=600)
    collected = {line.strip() for line in r.stdout.splitlines() if "::" in line}
    assert collected, "nothing collected:\n" + r.stdout[-2000:] + r.stderr[-2000:]
    functions = {c.split("[")[0] for c in collected}
    unknown = [t for t in ids if t not in collected and t not in functions]
    assert not unknown, "PARITY names tests that do not exist:\n  " + "\n  ".join(unknown)
