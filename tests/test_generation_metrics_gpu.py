"""GPU: what a generation run says about its own output, on the device.  metric.pair_stats / metric.diversity against the numpy
restatement (tests/pairstats_ref.py) reducing the device's own fp32 similarity matrix - integers exact, float64 sums within the
recursive-summation bound; evaluation.evaluate_generated on the recorded generation trials of tests/golden/evaluate.npz (gen_prefix,
gen_tokens: how many rows decode is the reference's own record) and on a batch without a valid row; evaluation.GenerationTotals over
several batches, with a planted duplicate and with a corpus; sampling.run_generation(get_metric=True) replaying the recorded tokens,
which must number and write its files exactly as the run without metrics; one pass with the real `generate` on the tiny model."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate_ref as ev  # noqa: E402
import pairstats_ref as pr  # noqa: E402
from musediffusion_amd import evaluation, metric, sampling  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402
from test_evaluate_cpu import fixture  # noqa: E402
from test_evaluate_gpu import _fatal, dev, library_launches  # noqa: E402
from test_pairstats_cpu import gen_batches  # noqa: E402

DEV = "cuda"


def matrix(vec, keys=None):
    """the device's fp32 similarity matrix (two-set call of the nearest-neighbour kernel: nothing masked, the diagonal as computed)"""
    vec = dev(vec)
    return metric.nearest(vec, vec.clone() if keys is None else dev(keys), return_sim=True)[1].cpu().numpy()


def host(st):
    return st.sum.cpu().numpy(), st.count.cpu().numpy(), st.nan.cpu().numpy(), None if st.above is None else st.above.cpu().numpy()


def judge(got, want, sim, on):
    total, count, nan, above = got
    w_total, w_count, w_nan, w_above = want
    assert np.array_equal(count, w_count) and np.array_equal(nan, w_nan)
    assert (above is None and w_above is None) or np.array_equal(above, w_above)
    assert (np.abs(total - w_total) <= pr.gamma(count) * pr.abs_rows(sim, on)).all()


# ------------------------------------------------------------------------------------------------ metric.pair_stats / diversity
def test_pair_stats_and_diversity_against_the_restatement():
    n = 300
    v = ev.unit_vectors(np.random.default_rng(31), n)
    v[200] = v[3]
    v[17, 44:] = np.nan
    sim = matrix(v)
    mask = np.arange(n) % 5 != 1
    groups = (np.arange(n) % 3 - 1).astype(np.int64)                                      # -1, 0, 1: any integer dtype, any sign
    for valid, grp, thr in ((None, None, None), (mask, None, pr.DEFAULT_THRESHOLD), (None, groups, 0.0), (mask, groups, pr.DEFAULT_THRESHOLD)):
        st = metric.pair_stats(dev(v), valid=None if valid is None else dev(valid), groups=None if grp is None else dev(grp), threshold=thr)
        assert st.sum.dtype == torch.float64 and st.count.dtype == st.nan.dtype == torch.int32 and st.sum.shape == st.count.shape == (n,)
        assert (st.above is None) == (thr is None) and (thr is None or st.above.dtype == torch.int32)
        on = pr.counted(n, n, valid, valid, grp, grp, True)
        judge(host(st), pr.reduce_rows(sim, on, thr), sim, on)
        # an int mask is a bool mask
        if valid is not None:
            again = metric.pair_stats(dev(v), valid=dev(valid.astype(np.int32) * 7), groups=None if grp is None else dev(grp.astype(np.int32)), threshold=thr)
            assert all(torch.equal(a, b) for a, b in zip((st.sum, st.count, st.nan, st.above), (again.sum, again.count, again.nan, again.above)))
        div, row_mean = metric.diversity(dev(v), None if valid is None else dev(valid), None if grp is None else dev(grp))
        assert div.dtype == torch.float64 and div.dim() == 0 and div.is_cuda and row_mean.dtype == torch.float64 and row_mean.shape == (n,)
        w_total, w_count, _, _ = pr.reduce_rows(sim, on)
        pairs = int(w_count.sum())
        tol = 2 * float(pr.gamma(pairs)) * float(pr.abs_rows(sim, on).sum()) / pairs + 4 * pr.U
        assert abs(float(div) - (1 - math.fsum(w_total.tolist()) / pairs)) <= tol and 0 < float(div) < 1
        some = w_count > 0
        got = row_mean.cpu().numpy()
        assert np.isnan(got[~some]).all() and (~some).any()                               # the NaN row, the masked rows: 0 / 0
        want = w_total[some] / w_count[some]
        assert (np.abs(got[some] - want) <= pr.gamma(w_count[some]) * pr.abs_rows(sim, on)[some] / w_count[some] + 2 * pr.U * np.abs(want)).all()
    st = metric.pair_stats(dev(v), threshold=pr.DEFAULT_THRESHOLD)
    assert st.above.sum().item() == 2 and st.above[3].item() == 1 and st.above[200].item() == 1
    # two sets
    k = ev.unit_vectors(np.random.default_rng(32), 70)
    k[6] = v[9]
    kmask, kgrp = np.arange(70) % 4 != 0, (np.arange(70) % 3 - 1).astype(np.int32)
    sim2 = matrix(v, k)
    st = metric.pair_stats(dev(v), dev(k), valid=dev(mask), keys_valid=dev(kmask), groups=dev(groups), keys_groups=dev(kgrp), threshold=pr.DEFAULT_THRESHOLD)
    on = pr.counted(n, 70, mask, kmask, groups, kgrp)
    judge(host(st), pr.reduce_rows(sim2, on, pr.DEFAULT_THRESHOLD), sim2, on)
    assert on[9, 6] and st.above[9].item() == 1 and st.above.sum().item() == 1
    # no counted pair: NaN, not an error
    div, row_mean = metric.diversity(dev(v[:4]), dev(np.array([0, 1, 0, 0])))
    assert math.isnan(float(div)) and torch.isnan(row_mean).all()
    with pytest.raises(AssertionError):
        metric.pair_stats(dev(v), keys_groups=dev(groups))


# ------------------------------------------------------------------------------------------------ evaluate_generated
def invalid_batch():
    """eight recorded rows that do not decode"""
    rows, mask = [], None
    for tokens, mask in gen_batches():
        m = pr.evaluate_generated(tokens, mask)
        rows += [tokens[b] for b in np.flatnonzero(~m["valid"])]
    return np.stack(rows[:8]), mask


def test_evaluate_generated_on_the_recorded_trials():
    f = fixture()
    for n, (tokens, mask) in enumerate(gen_batches()):
        want = pr.evaluate_generated(tokens, mask)
        m = evaluation.evaluate_generated(dev(tokens), dev(mask))
        assert int(m.valid_count) == int(f["gen_counts"][n]) == want["valid_count"] and int(m.fatal) == 0
        assert m.valid.dtype == torch.bool and m.valid_count.dtype == torch.int64 and m.counts.dtype == torch.int64 and m.vec.shape == (8, 56)
        assert np.array_equal(m.valid.cpu().numpy(), want["valid"]) and tuple(m.counts.tolist()) == want["counts"]
        v = want["valid"]
        assert np.allclose(m.vec.cpu().numpy()[v], want["vec"][v], rtol=1e-5, atol=1e-12, equal_nan=True)
        rows = m.decoded.cpu()                                                            # the driver writes from this decode
        assert np.array_equal(rows.status == du.OK, v)
    tokens, mask = invalid_batch()
    m = evaluation.evaluate_generated(dev(tokens), dev(mask))
    assert int(m.valid_count) == 0 and not m.valid.any() and m.counts.tolist() == [0, 0, 0, 0] and int(m.fatal) == 0
    s = evaluation.GenerationTotals(DEV).update(m).summary()
    assert s["valid"] == 0 and s["pairs"] == 0 and s["nan_pairs"] == 0 and all(math.isnan(s[k]) for k in ("diversity", "duplicates", "cp", "cv"))
    bad = gen_batches()[0][0].copy()
    row = int(np.flatnonzero(pr.evaluate_generated(bad, mask)["valid"])[0])
    bad[row, 2] = 640                                                                      # a time-signature token out of range: BAD_META
    assert pr.evaluate_generated(bad, mask)["fatal"] == du.BAD_META
    m = evaluation.evaluate_generated(dev(bad), dev(mask))
    assert int(m.fatal) == du.BAD_META and not bool(m.valid[row])
    with pytest.raises(KeyError):
        evaluation.GenerationTotals(DEV).update(m).summary()


def test_launch_count_does_not_depend_on_the_batch_size():
    f = fixture()
    tokens = f["gen_tokens"]
    mask = np.tile(gen_batches()[0][1][:1], (24, 1))
    counts = {}
    for B in (2, 24):
        args = (dev(tokens[:B]), dev(mask[:B]))
        evaluation.evaluate_generated(*args)                                              # warm
        counts[B] = library_launches(lambda: evaluation.evaluate_generated(*args))
    assert sorted(counts[2]) == sorted(counts[24]) and counts[2], counts
    m = evaluation.evaluate_generated(dev(tokens), dev(mask))
    totals = evaluation.GenerationTotals(DEV, corpus=m.vec).update(m)
    names = library_launches(totals.summary)                                               # one pair-statistics launch, one nearest launch
    assert len([k for k in names if k.startswith("msim_pair_stats_kernel")]) == 1, names
    assert len([k for k in names if k.startswith("msim_nearest_kernel")]) == 1 and not [k for k in names if "gemm" in k.lower()], names


# ------------------------------------------------------------------------------------------------ GenerationTotals
def run_totals(batches, groups=False, corpus=None, corpus_valid=None, threshold=None):
    """the device totals and the restatement fed with the device's own vectors, masks and counts -> (summary, want, tol)"""
    kw = {} if threshold is None else {"duplicate_threshold": threshold}
    totals = evaluation.GenerationTotals(DEV, corpus=None if corpus is None else dev(corpus),
                                         corpus_valid=None if corpus_valid is None else dev(corpus_valid), **kw)
    ref = pr.GenTotals(corpus=corpus, corpus_valid=corpus_valid, **kw)
    for n, (tokens, mask) in enumerate(batches):
        m = evaluation.evaluate_generated(dev(tokens), dev(mask))
        g = np.full(len(tokens), n - 1, np.int32) if groups else None
        totals.update(m, None if g is None else dev(g))
        ref.update(m.vec.cpu().numpy(), m.valid.cpu().numpy(), m.counts.cpu().numpy(), g)
    vec = np.concatenate(ref.vec)
    want, tol = ref.summary(sim=matrix(vec), corpus_sim=None if corpus is None else matrix(vec, corpus))
    return totals.summary(), want, tol, totals


def compare(s, want, tol):
    assert set(s) == set(want)
    for key in ("valid", "pairs", "nan_pairs"):
        assert s[key] == want[key] and isinstance(s[key], int), key
    for key in ("duplicates", "cp", "cv", "memorised"):                                    # ratios of equal integers: the same division
        assert key not in want or s[key] == want[key] or (math.isnan(s[key]) and math.isnan(want[key])), key
    for key in ("diversity", "novelty"):
        assert key not in want or abs(s[key] - want[key]) <= tol[key], (key, s[key], want[key], tol[key])


def test_totals_over_several_batches():
    batches = gen_batches()
    s, want, tol, totals = run_totals(batches)
    compare(s, want, tol)
    assert s["valid"] == 14 and s["pairs"] + s["nan_pairs"] == 14 * 13 // 2 and 0 < s["diversity"] < 1 and s["duplicates"] == 0
    assert totals.summary() == s                                                           # the same call, the same bits
    host_counts = np.sum([pr.evaluate_generated(t, m)["counts"] for t, m in batches], axis=0)
    assert s["cp"] == host_counts[1] / host_counts[0] and s["cv"] == host_counts[3] / host_counts[2]
    # one group per batch: only pairs within a batch count
    sg, want, tol, _ = run_totals(batches, groups=True)
    compare(sg, want, tol)
    assert sg["pairs"] + sg["nan_pairs"] == sum(int(c) * (int(c) - 1) // 2 for c in fixture()["gen_counts"]) and sg["valid"] == 14


def test_totals_with_a_planted_exact_duplicate():
    tokens, mask = gen_batches()[2]
    valid = np.flatnonzero(pr.evaluate_generated(tokens, mask)["valid"])
    twice = tokens.copy()
    twice[valid[1]] = twice[valid[0]]
    s, want, tol, _ = run_totals([gen_batches()[1], (twice, mask)])
    compare(s, want, tol)
    assert s["duplicates"] == 2 / s["valid"] > 0 and s["diversity"] < 1 and s["valid"] == 12
    # the threshold is the caller's: above every similarity nothing is a duplicate
    s2, want, tol, _ = run_totals([gen_batches()[1], (twice, mask)], threshold=1.5)
    compare(s2, want, tol)
    assert s2["duplicates"] == 0 and s2["diversity"] == s["diversity"]


def test_totals_with_a_corpus_that_holds_a_generated_row():
    batches = gen_batches()
    m = evaluation.evaluate_generated(dev(batches[2][0]), dev(batches[2][1]))
    row = int(np.flatnonzero(m.valid.cpu().numpy())[0])
    corpus = ev.unit_vectors(np.random.default_rng(33), 200)
    corpus[150] = m.vec[row].cpu().numpy()
    corpus[7, 44:] = np.nan                                                                # a corpus piece without notes: masked below
    cv = np.ones(200, bool)
    cv[7] = False
    s, want, tol, _ = run_totals(batches, corpus=corpus, corpus_valid=cv)
    compare(s, want, tol)
    assert s["memorised"] >= 1 / 14 > 0 and 0 < s["novelty"] < 1
    cv[150] = False                                                                        # without the copied piece nothing is memorised
    s2, want, tol, _ = run_totals(batches, corpus=corpus, corpus_valid=cv)
    compare(s2, want, tol)
    assert s2["memorised"] < s["memorised"] and s2["novelty"] > s["novelty"]


# ------------------------------------------------------------------------------------------------ the driver
def test_run_generation_with_metrics_writes_what_the_plain_run_writes(tmp_path):
    f = fixture()
    L = f["gen_tokens"].shape[1]
    reps, logs = {}, {}
    for on in (False, True):
        trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
        logs[on] = []
        reps[on] = sampling.run_generation(None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=6, out_dir=str(tmp_path / str(on)),
                                           sampler=lambda cond: next(trials), log=logs[on].append, get_metric=on)
        assert len(list(trials)) == 1                                                      # 2, then 2 + 5 >= 6: both stop after the second trial
        logs[on] = [ln.replace(str(tmp_path / str(on)), "<out>") for ln in logs[on]]
    off, rep = reps[False], reps[True]
    assert (rep.total_valid_count, rep.batches) == (off.total_valid_count, off.batches) == (7, 2)
    names = sorted(os.listdir(tmp_path / "True"))
    assert names == sorted(os.listdir(tmp_path / "False")) == [str(x) for x in f["gen_names"][:7]]
    for name in names:
        assert open(tmp_path / "True" / name, "rb").read() == open(tmp_path / "False" / name, "rb").read()
    assert off.totals is None and off.summary is None
    extra = [ln for ln in logs[True] if ln not in logs[False]]
    assert [ln for ln in logs[True] if ln in logs[False]] == logs[False]
    assert extra == ["### with calculating metrics ...", evaluation.generation_block(rep.summary)] and " Summary: Generation " in extra[1]
    assert isinstance(rep.totals, evaluation.GenerationTotals) and rep.totals.summary() == rep.summary
    s, want, tol, _ = run_totals(gen_batches()[:2])
    compare(rep.summary, want, tol)
    assert rep.summary == s and rep.summary["valid"] == 7 and "novelty" not in rep.summary
    # with a corpus and a threshold of the caller's, without an output directory
    trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
    corpus = ev.unit_vectors(np.random.default_rng(34), 50)
    rep = sampling.run_generation(None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=100, out_dir=None, max_batches=3,
                                  sampler=lambda cond: next(trials), log=lambda s: None, get_metric=True, corpus=dev(corpus), duplicate_threshold=0.0)
    s, want, tol, _ = run_totals(gen_batches(), corpus=corpus, threshold=0.0)
    compare(rep.summary, want, tol)
    assert rep.total_valid_count == 14 and rep.summary["memorised"] == 1 and rep.summary["duplicates"] == 1     # everything reaches 0


def test_run_generation_with_metrics_and_the_real_sampler(tmp_path, monkeypatch):
    """one pass with the default sampler on the tiny oracle model, two batches: the tokens are garbage and mostly invalid, which is the
    point - the loop ends, max_batches holds, the summary is filled.  A row on which the reference's decode raises (a fatal status) must
    raise here too: the test decodes the tokens the sampler returned itself to know which of the two to expect."""
    from test_diffusion_gpu import build
    m, diff, _, inp, c = build("tiny")
    diff.noise_fn, diff.rng_mode = None, "philox"
    torch.manual_seed(11)
    seen = []
    real = sampling.generate
    monkeypatch.setattr(sampling, "generate", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    meta = inp["batch"]["correct_ids"][0, :11].tolist()
    try:
        rep = sampling.run_generation(m, diff, meta, batch_size=c["B"], seq_len=c["L"], num_samples=1000, step=10, out_dir=str(tmp_path / "g"),
                                      max_batches=2, log=lambda s: None, get_metric=True)
    except (IndexError, KeyError, RuntimeError):
        rep = None
    cond = du.meta_to_batch(meta, c["B"], c["L"])
    assert 1 <= len(seen) <= 2
    if any(_fatal(t, cond["input_mask"], False) for t in seen):
        assert rep is None
    else:
        s = rep.summary
        assert rep.batches == 2 and len(seen) == 2 and rep.total_valid_count == len(os.listdir(tmp_path / "g")) == s["valid"] <= 2 * c["B"]
        assert s["pairs"] + s["nan_pairs"] == s["valid"] * (s["valid"] - 1) // 2
        assert all(math.isnan(s[k]) or 0 <= s[k] <= 1 for k in ("duplicates", "cp", "cv"))
        assert math.isnan(s["diversity"]) == (s["pairs"] == 0)
