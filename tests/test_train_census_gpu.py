"""Launch census of the training kernels (csrc/train.hip): every kernel - and every path of one that a runtime argument selects - the
product launches in a training step must be compared with a reference by some test.  The census records the GEMM census' three training
micro-steps (both tapes), the seq_len 128 step again in fp32 and one optimizer step with the library's per-launch recorder, turns each
train.hip launch into a key (tests/train_census.py: census_key) and looks it up in PARITY.  A new dispatch branch, or a production shape
that starts taking another path, fails here until a parity case reaches it.

PARITY maps each key to the tests that compare it with a reference: `module::test[id]` for one case, `module::test` for all of a test's
cases.  The LayerNorm, column-sum, scatter and head-permute entries are generated from the parity matrix' own case lists: each of those
cases records its launch and asserts the very keys it is listed under here.  So are the optimizer step's: one key per number of EMA copies
(tests/train_census.py: ADAM_KEYS), from the case list of the optimizer matrix (tests/test_optim_matrix_gpu.py), which also holds the norm
and clip kernels' cases.  Second entries name older direct comparisons, each against a reference and not against another launch of the
same kernel: weight_prep_kernel against torch's casts (row-major; the panel forms in the matrix), sum_slices_kernel against a matmul of the
rounded inputs, the optimizer kernels through FusedAdamWEMA against torch.optim.AdamW, the reference's update_ema and torch's
clip_grad_norm_ on the CPU."""
import os
import subprocess
import sys

import pytest

import test_optim_matrix_gpu as om
import test_train_matrix_gpu as tm
import train_census as tc

M = "tests/test_train_matrix_gpu.py::"
OM = "tests/test_optim_matrix_gpu.py::"
OPTIM = "tests/test_optim_gpu.py::"

PARITY = {}


def _add(key, test):
    if test not in PARITY.setdefault(key, []):
        PARITY[key].append(test)


for _c in tm.LN_CASES:
    for _k in tm.ln_case_keys(_c):
        _add(_k, M + "test_layernorm_backward[%s]" % tm._ln_id(_c))
for _c in tm.COLSUM_CASES:
    for _k in tm.colsum_case_keys(_c):
        _add(_k, M + "test_column_sums[%s]" % tm._colsum_id(_c))
for _n, _E, _V, _ in tm.SCATTER_CASES:
    _add(tc.scatter_key(32 if _n >= 8192 else (_n + 255) // 256, _E), M + "test_scatter_add_rows")
for _mode, _, _, _, _, _, _kernel in tm.HP_CASES:
    _add("%s | mode=%d" % (_kernel, _mode), M + "test_head_permute_bit_for_bit")
for _T in ("bf16", "float"):
    _add("act_fwd_kernel<%s>" % _T, M + "test_activation_forward_and_backward")
    _add("act_bwd_kernel<%s>" % _T, M + "test_activation_forward_and_backward")
    _add("add_inplace_kernel<%s>" % _T, M + "test_add_inplace_bit_for_bit")
    _add("add_pos_time_kernel<%s>" % _T, M + "test_add_pos_time_bit_for_bit")
    _add("ce_bwd_kernel<%s>" % _T, M + "test_cross_entropy_backward")
    _add("softmax_rows_kernel<%s>" % _T, M + "test_softmax_rows_forward_and_backward")
    _add("softmax_bwd_rows_kernel<%s>" % _T, M + "test_softmax_rows_forward_and_backward")
    _add("transpose_kernel<%s>" % _T, M + "test_transpose_bit_for_bit")
for _k, _t in {
    "add_pos_time8_kernel": M + "test_add_pos_time_bit_for_bit",
    "transpose64_kernel": M + "test_transpose_bit_for_bit",
    "ce_fwd_kernel": M + "test_cross_entropy_forward",
    "sqdiff_mean_kernel | vec=0": M + "test_squared_error_mean",
    "sqdiff_mean_kernel | vec=1": M + "test_squared_error_mean",
    "sqdiff_bwd_kernel": M + "test_squared_error_backward",
    "scale_rows_kernel": M + "test_scale_rows",
    "scatter_rows_final_kernel": M + "test_scatter_add_rows",
    "repack_panel_kernel": M + "test_repack_panel_each_direction",
    "sum_slices_kernel": M + "test_sum_slices_against_float64",
    "weight_prep_kernel": M + "test_weight_prep_panel_forms",
    "sumsq_chunks_kernel": OM + "test_grad_norm",
    "sum_partials_kernel": OM + "test_grad_norm",
    "clip_grads_kernel": OM + "test_clip_grads",
}.items():
    _add(_k, _t)
# the optimizer step: one key per adamw_ema_chunk<NEMA> instantiation, each case of the optimizer matrix under the n_ema it asserts it ran
assert {_c[2] for _c in om.ADAM_CASES} == set(range(5))
for _c in om.ADAM_CASES:
    _add(tc.adam_key(_c[2]), OM + "test_adamw_ema_step[%s]" % om._id(_c))
# (second entries: the older comparisons with torch.optim.AdamW, update_ema and clip_grad_norm_ through FusedAdamWEMA)
for _k in (tc.adam_key(3), "sumsq_chunks_kernel", "sum_partials_kernel"):
    _add(_k, OPTIM + "test_fused_adamw_ema_matches_torch")
for _k in (tc.adam_key(1), "clip_grads_kernel"):
    _add(_k, OPTIM + "test_parameters_without_a_gradient_are_skipped_like_torch_adamw")
_add("sum_slices_kernel", "tests/test_kernels_gpu.py::test_gemm_dw_k_major")
_add("weight_prep_kernel", "tests/test_kernels_gpu.py::test_weight_prep_one_launch_copies_and_transposes")


@pytest.mark.gpu
def test_every_launched_training_kernel_has_a_parity_test():
    import torch
    dev = torch.device("cuda", 0)
    seen = {}
    for name, run in tc.WORKLOADS.items():
        recs = run(dev)
        # (an empty record would make the census pass vacuously: launches that bypass the recorder, a graph replay)
        assert recs, "workload %r recorded no train.hip launch" % name
        for key, note, grid in recs:
            seen.setdefault(key, [0, set(), note, grid])
            seen[key][0] += 1
            seen[key][1].add(name)
        torch.cuda.empty_cache()
    print("\n%-72s %6s  %s" % ("training kernel launched (census key)", "calls", "parity tests / workloads"))
    for key in sorted(seen):
        n, names, note, grid = seen[key]
        print("%-72s %6d  %s" % (key, n, "%d test(s), e.g. %s" % (len(PARITY[key]), PARITY[key][0].split("::")[1]) if key in PARITY else "NONE"))
        print("%-72s %6s  %s | e.g. %s grid=%d" % ("", "", ", ".join(sorted(names)), note or "-", grid))
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
    # a key of every kernel of the family: a kernel the table cannot name at all would be a hole in census_key
    named = {k.split("<")[0].split(" |")[0].strip() for k in PARITY}
    assert named == set(tc.FAMILY), sorted(set(tc.FAMILY) ^ named)
