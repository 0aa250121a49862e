"""Launch census of the sampling step's kernels outside the GEMMs and attention (csrc/elementwise.hip, csrc/norm.hip, csrc/rounding.hip,
csrc/headtail.hip, the two rounding helpers of csrc/gemm.hip): every kernel - and every path of one that a runtime argument selects -
the product launches in a forward, a reverse step or a whole generation must be compared with a reference by some test.  The census
records tests/step_census.py's workloads (the three forwards, a p and a ddim step of config 2, the p step with each fusion switched off,
a generation and a modification from ids to tokens) with the library's per-launch recorder, turns each launch of the family into a key
(step_census.census_key) and looks it up in PARITY.  A new dispatch branch, or a production shape that starts taking another path, fails
here until a parity case reaches it.

PARITY maps each key to the tests that compare it with a reference: `module::test[id]` for one case, `module::test` for all of a test's
cases.  Its entries are generated from the parity matrix' own case lists (tests/test_step_matrix_gpu.py): each of those cases records its
launch and asserts the very key it is listed under here.  The distance-logit argmax points at tests/test_distance_matrix_gpu.py.
spin_kernel (mh_stream_delay) idles a wave for a time and has no result to compare: exempt."""
import os
import subprocess
import sys

import pytest

import step_census as sc
import test_step_matrix_gpu as sm

M = "tests/test_step_matrix_gpu.py::"
PARITY = {}


def _add(key, test):
    if test not in PARITY.setdefault(key, []):
        PARITY[key].append(test)


for _c in sm.EPI_CASES:
    _add(sm.epi_case_key(_c), M + "test_update_kernels_bit_for_bit[%s]" % sm._epi_id(_c))
_add(sm.epi_case_key(sm.EPI_BIG), M + "test_update_kernel_second_sweep")
for _c in sm.SLOT_CASES:
    _add(sm.slot_case_key(_c), M + "test_update_with_slot_fold_bit_for_bit[%s]" % sm._slot_id(_c))
for _c in sm.LN_CASES:
    _add(sm.ln_case_key(_c), M + "test_layernorm_rows[%s]" % sm._ln_id(_c))
for _c in sm.LN_ADD_CASES:
    _add(sm.ln_add_case_key(_c), M + "test_add_pos_time_layernorm_rows[%s]" % sm._ln_add_id(_c))
for _c in sm.PANEL_CASES:
    _add(sm.panel_case_key(_c), M + "test_layernorm_panel[%s]" % sm._panel_id(_c))
for _c in sm.PANEL16_DBG_CASES:
    _add(sm.panel_case_key(_c), M + "test_layernorm_panel_16_row_form[%s]" % sm._panel_id(_c))
for _c in sm.UPD_CASES:
    _add(sm.upd_case_key(_c), M + "test_down_proj_round_fused_with_update[%s]" % sm._upd_id(_c))
for _H in (512, 768):
    _add(sc.tail_key(sm.ROUND_KERNEL[_H], 0), M + "test_down_proj_round_fused")
for _H in (256, 512, 768):
    _add(sm.TAIL_KERNEL[_H], M + "test_down_proj_fused")
    _add(sm.HEAD_KERNEL[_H], M + "test_up_proj_ln_fused")
for _T in ("bf16", "float"):
    _add("cast_pad_kernel<%s>" % _T, M + "test_casts_and_panel_movers_bit_for_bit")
    _add("cast_to_f32_kernel<%s>" % _T, M + "test_casts_and_panel_movers_bit_for_bit")
    _add("timestep_embedding_kernel<%s>" % _T, M + "test_timestep_embedding")
for _k, _t in {
    "pack_panel_kernel": "test_casts_and_panel_movers_bit_for_bit",
    "unpack_panel_kernel": "test_casts_and_panel_movers_bit_for_bit",
    "q_sample_kernel": "test_q_sample_bit_for_bit",
    "embed_gather_kernel": "test_embed_gather_bit_for_bit",
    "row_sqnorm_kernel": "test_row_sqnorm",
    "row_sqnorm_f32_kernel": "test_round_to_embedding_mfma",
    "argbest_reduce_kernel": "test_round_to_embedding_mfma",
    "round_split_kernel": "test_round_split_table",
    "distance_scores_kernel": "test_distance_scores_bit_for_bit",
    "trunc_normal_kernel": "test_trunc_normal_against_host_restatement",
    "step_begin_kernel": "test_loop_state_kernels",
    "step_end_kernel": "test_loop_state_kernels",
    "step_advance_kernel": "test_loop_state_kernels",
    "vocab_argmax_kernel<0>": "test_vocab_argmax",
    "vocab_argmax_kernel<1>": "test_vocab_argmax",
}.items():
    _add(_k, M + _t)
_add("trunc_normal_kernel", M + "test_trunc_normal_layout")
_add("vocab_argmax_kernel<2>", "tests/test_distance_matrix_gpu.py::test_distance_argmax_against_float64")
_add("vocab_argmax_kernel<2>", "tests/test_distance_matrix_gpu.py::test_distance_argmax_returns_the_first_index_of_a_tie")


@pytest.mark.gpu
def test_every_launched_step_kernel_has_a_parity_test():
    import torch
    dev = torch.device("cuda", 0)
    seen = {}
    for name, run in sc.WORKLOADS.items():
        recs = run(dev)
        # (an empty record would make the census pass vacuously: launches that bypass the recorder, a graph replay)
        assert recs, "workload %r recorded no launch of the family" % name
        for key, note, grid in recs:
            seen.setdefault(key, [0, set(), note, grid])
            seen[key][0] += 1
            seen[key][1].add(name)
        torch.cuda.empty_cache()
    print("\n%-100s %6s  %s" % ("step kernel launched (census key)", "calls", "parity tests / workloads"))
    for key in sorted(seen):
        n, names, note, grid = seen[key]
        print("%-100s %6d  %s" % (key, n, "%d test(s), e.g. %s" % (len(PARITY[key]), PARITY[key][0].split("::")[1]) if key in PARITY else
                                  ("exempt" if key in sc.EXEMPT else "NONE")))
        print("%-100s %6s  %s | e.g. %s grid=%d" % ("", "", ", ".join(sorted(names)), note or "-", grid))
    missing = sorted(k for k in seen if k not in PARITY and k not in sc.EXEMPT)
    assert not missing, "launched by the product, covered by no parity test:\n  " + "\n  ".join(missing)


def test_parity_table_names_existing_tests():
    """every test PARITY names is collected (pytest --collect-only over the modules it names; nothing runs), and every kernel of the
    family has a key"""
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
    named = {k.split("<")[0].split(" |")[0].strip() for k in PARITY}
    assert named == set(sc.FAMILY) - set(sc.EXEMPT), sorted((set(sc.FAMILY) - set(sc.EXEMPT)) ^ named)
