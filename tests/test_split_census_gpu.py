"""Launch census of the split-precision kernels (csrc/split.hip, compute_dtype "bf16x3" / "f16x3"): every kernel - and every path of one
that a runtime argument selects - the product launches in a split-mode forward must be compared with a float64 reference by some case of
the parity matrix.  The census records the sampler's forward at the bench.py shapes `c2`, `c2-bertbase` (hidden size 768: the unfused
out=2 GEMM followed by split_layernorm) and `c1` in both split modes, eager, with the library's per-launch recorder, turns each split.hip
launch into a key (tests/split_census.py: census_key - the part type and the path classes come from the launch note, the persistent class
from the note's tile count against the launched grid) and looks it up in PARITY.  A new dispatch branch, or a production shape that starts
taking another path, fails here until a parity case reaches it.  No key is exempt.

PARITY is generated from the matrix' own case lists (tests/test_split_matrix_gpu.py): each case records its launch and asserts the very
key it is listed under here.  The GEMM census (tests/test_gemm_census_gpu.py) and the attention census
(tests/test_attention_census_gpu.py) keep their own, coarser keys for split_gemm_kernel, split_gemm_ln_kernel and split_attn_kernel and
the older cases those point at: their workloads are a subset of this census', and the launches are covered a second time here."""
import os
import subprocess
import sys

import pytest

import split_census as sc
import split_ref as sr
import test_split_matrix_gpu as tm

M = "tests/test_split_matrix_gpu.py::"

PARITY = {}


def _add(key, test):
    if test not in PARITY.setdefault(key, []):
        PARITY[key].append(test)


for _dt in sr.DTYPES:
    _n = sr.NAME[_dt]
    for _c in tm.MOVER_CASES:
        _add(sc.mover_key("pack", _n, _c[1]), M + "test_pack_bit_for_bit[%s-%s]" % (tm._mover_id(_c), _n))
        _add(sc.mover_key("join", _n, _c[1]), M + "test_join_bit_for_bit[%s-%s]" % (tm._mover_id(_c), _n))
    for _c in tm.LN_CASES:
        _add(sc.ln_key(_n, _c[3], _c[0]), M + "test_layernorm[%s-%s]" % (tm._ln_id(_c), _n))
    for _c in tm.GEMM_CASES:
        _add(tm.gemm_case_key(_c, _dt), M + "test_gemm[%s-%s]" % (tm._gemm_id(_c), _n))
    for _K, _M in tm.GEMM_LN_CASES:
        _add(sc.gemm_ln_key(_n, _K), M + "test_gemm_residual_layernorm[%d-%d-%s]" % (_K, _M, _n))
    for _c in tm.ATTN_CASES:
        _add(sc.attn_key(_n, _c[0], _c[1]), M + "test_attention[%s-%s]" % (tm._attn_id(_c), _n))


@pytest.mark.gpu
def test_every_launched_split_kernel_has_a_parity_test():
    import torch
    dev = torch.device("cuda", 0)
    seen = {}
    for name, run in sc.WORKLOADS.items():
        recs = run(dev)
        # (an empty record would make the census pass vacuously: launches that bypass the recorder, a graph replay)
        assert recs, "workload %r recorded no split.hip launch" % name
        for key, note, grid in recs:
            seen.setdefault(key, [0, set(), note, grid])
            seen[key][0] += 1
            seen[key][1].add(name)
        torch.cuda.empty_cache()
    print("\n%-100s %6s  %s" % ("split kernel launched (census key)", "calls", "parity tests / workloads"))
    for key in sorted(seen):
        n, names, note, grid = seen[key]
        print("%-100s %6d  %s" % (key, n, "%d test(s), e.g. %s" % (len(PARITY[key]), PARITY[key][0].split("::")[1]) if key in PARITY else "NONE"))
        print("%-100s %6s  %s | e.g. %s grid=%d" % ("", "", ", ".join(sorted(names)), note or "-", grid))
    missing = sorted(k for k in seen if k not in PARITY)
    assert not missing, "launched by the product, covered by no parity test:\n  " + "\n  ".join(missing)


def test_parity_table_names_existing_tests():
    """every test PARITY names is collected (pytest --collect-only over the module it names; nothing runs)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ids = sorted({t for tests in PARITY.values() for t in tests})
    modules = sorted({t.split("::")[0] for t in ids})
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", "-m", "gpu or not gpu", *modules],
                       cwd=repo, capture_output=True, text=True, timeout=600)
    collected = {line.strip() for line in r.stdout.splitlines() if "::" in line}
    assert collected, "nothing collected:\n" + r.stdout[-2000:] + r.stderr[-2000:]
    unknown = [t for t in ids if t not in collected]
    assert not unknown, "PARITY names tests that do not exist:\n  " + "\n  ".join(unknown[:20])
    # a key of every kernel of the family: a kernel the table cannot name at all would be a hole in census_key
    named = {k.split("<")[0].strip() for k in PARITY}
    assert named == set(sc.FAMILY), sorted(set(sc.FAMILY) ^ named)
