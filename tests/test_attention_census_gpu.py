"""Launch census of the attention family: every attention kernel variant the product launches at the bench.py shapes must be compared
with a reference by some test.  The census records the GEMM census' eager runs (sampler forward in four compute modes, bert-base, one
reverse step, training micro-steps on both tapes) plus one forward at the reference's own shape (seq_len 2096) with the library's
per-launch recorder, turns each attention launch into a key (tests/attention_census.py: census_key - the launch note names the
instantiation) and looks it up in PARITY.  A new dispatch branch, or a production shape that starts launching another variant, fails here
until a parity case reaches it.

It also asserts what the multi-item cases of the parity matrix rest on: at the shapes bench.py times, the streaming kernels launch fewer
blocks than they have items, so every block walks several (batch, head, block) items.

PARITY maps each key to the tests that compare that variant with a reference: `module::test[id]` for one case, `module::test` for all of
a test's cases."""
import os
import subprocess
import sys

import pytest

import attention_census as ac

M = "tests/test_attention_matrix_gpu.py::"
FWD = M + "test_forward_variant_against_reference[%s]"
BWD = M + "test_backward_variant_against_reference[%s]"
SMALL = ["tests/test_kernels_gpu.py::test_attention"]


def _fwd(variant, dh, *cases):
    return [FWD % ("%s-dh%d-%s" % (variant, dh, c)) for c in cases]


def _bwd(dh, drop, full, panel):
    """the backward pair <dh, DROP, FULL> with row-major (panel 0) or panel O / dQ | dK | dV; both kernels of a pair share their cases"""
    p = "-p0.1" if drop else ""
    p784 = "-p0.5" if drop and dh == 64 else p
    if full:
        cases = ["small-L512-heads-rows" + p, "multi-L512-tokens-rows" + p]
        if panel:
            cases = ["small-L1024-tokens-panel" + p] + (["multi-L1024-tokens-panel" + p] if dh == 64 else [])
    elif panel:
        cases = ["ragged-L784-tokens-panel" + p784] + (["ragged-L2096-tokens-panel" + p] if drop else ["multi-L528-tokens-panel"])
    else:
        cases = ["ragged-L528-heads-rows" + p] + (["multi-L528-tokens-rows" + p] if drop else ["ragged-L2096-tokens-rows"])
    tests = [BWD % ("dh%d-%s-%s-%s" % (dh, "drop" if drop else "plain", "full" if full else "bound", c)) for c in cases]
    if panel and not drop and (dh, full) in ((64, 0), (32, 1)):
        tests.append(M + "test_forward_then_backward_chained[%s]" % ("64-784" if dh == 64 else "32-1024"))
    return tests


PARITY = {}
for _dh in (64, 32):
    PARITY.update({
        ac.fwd_key(_dh, full=1, kvnt=1): _fwd("plain-full-kvnt", _dh, "small-L512-heads-rows-lse", "multi-L512-tokens-panel-lse"),
        ac.fwd_key(_dh, full=1): _fwd("plain-full", _dh, "small-L1024-tokens-rows", "multi-L1024-heads-panel-lse"),
        ac.fwd_key(_dh): _fwd("plain-bound", _dh, "ragged-L528-tokens-rows-lse", "ragged-L784-heads-panel", "ragged-L2096-tokens-panel-lse",
                              "multi-L528-tokens-rows-lse"),
        ac.fwd_key(_dh, full=1, kvnt=1, pre=1): _fwd("pre-kvnt", _dh, "small-L512-heads-rows", "multi-L512-heads-panel"),
        ac.fwd_key(_dh, full=1, pre=1): _fwd("pre", _dh, "small-L1024-heads-panel", "multi-L1024-heads-rows"),
        ac.fwd_key(_dh, nw=8, sk=128 if _dh == 64 else 256, dropv=1): _fwd(
            "drop-gen", _dh, "ragged-L528-tokens-rows-lse-p0.1", "ragged-L784-heads-panel-lse-p0.5", "small-L1024-tokens-panel-lse-p0.1",
            "multi-L512-tokens-rows-lse-p0.1"),
        ac.fwd_key(_dh, dropv=2): _fwd(
            "drop-read-bound", _dh, "ragged-L528-tokens-panel-lse-p0.1", "ragged-L2096-tokens-rows-lse-p0.1", "multi-L528-tokens-rows-lse-p0.1",
            *(["small-L1024-tokens-rows-lse-p0.1", "multi-L512-tokens-panel-lse-p0.1"] if _dh == 32 else [])),
    })
    for _drop in (0, 1):
        for _full in (0, 1):
            for _panel in (0, 1):
                for _key in ac.bwd_keys(_dh, _drop, _full, _panel):
                    PARITY[_key] = _bwd(_dh, _drop, _full, _panel)
PARITY[ac.fwd_key(64, dropv=2, full=1)] = _fwd("drop-read-full", 64, "small-L1024-tokens-rows-lse-p0.1", "multi-L1024-tokens-panel-lse-p0.1")
# the small-L kernels (seq_len < 512, head dims without a streaming build, fp32 parity mode) and the split-precision attention keep
# their own reference tests
PARITY.update({
    "attn_res_bf16_kernel<DH, 8> | kind=res8 dh=32": SMALL,
    "attn_res_bf16_kernel<DH, 8> | kind=res8 dh=64": SMALL,
    "attn_bf16_kernel<DH> | kind=tiled dh=32": SMALL,
    "attn_bf16_kernel<DH> | kind=tiled dh=64": SMALL,
    "attn_f32_kernel<DH> | kind=f32 dh=32": SMALL,
    "attn_f32_kernel<DH> | kind=f32 dh=64": SMALL,
    "split_attn_kernel<T, 64, 8>": ["tests/test_split_gpu.py::test_split_attention"],
    "split_attn_kernel<T, 64>": ["tests/test_split_gpu.py::test_split_attention"],
    "split_attn_kernel<T, 32>": ["tests/test_split_gpu.py::test_split_attention"],
    "attn_bwd_rowdot_kernel": ["tests/test_kernels_gpu.py::test_attention_stream_backward"],
})


@pytest.mark.gpu
def test_every_launched_attention_variant_has_a_parity_test():
    import torch
    dev = torch.device("cuda", 0)
    seen, single = {}, []
    for name, run in ac.WORKLOADS.items():
        recs = run(dev)
        # (an empty record would make the census pass vacuously: launches that bypass the recorder, a graph replay)
        assert recs or name in ac.NO_ATTENTION_KERNEL, "workload %r recorded no attention launch" % name
        for key, note, grid in recs:
            seen.setdefault(key, [0, set(), note, grid])
            seen[key][0] += 1
            seen[key][1].add(name)
            if name in ac.MULTI_ITEM and "items=" in note and not grid < ac.items(note):
                single.append("%s: %s grid=%d" % (name, note, grid))
        torch.cuda.empty_cache()
    print("\n%-86s %6s  %s" % ("attention variant launched (census key)", "calls", "parity tests / workloads"))
    for key in sorted(seen):
        n, names, note, grid = seen[key]
        print("%-86s %6d  %s" % (key, n, "%d test(s)" % len(PARITY[key]) if key in PARITY else "NONE"))
        print("%-86s %6s  %s | e.g. %s grid=%d" % ("", "", ", ".join(sorted(names)), note, grid))
    missing = sorted(k for k in seen if k not in PARITY)
    assert not missing, "launched by the product, covered by no parity test:\n  " + "\n  ".join(missing)
    assert not single, "streaming launches of the multi-item workloads with one item per block:\n  " + "\n  ".join(single)


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
