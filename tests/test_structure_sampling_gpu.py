"""GPU: the structure counts above the kernel.  metric.structure_counts on decode_tokens of every record of tests/golden/decode.npz
against the restatement on the reference's own recorded notes; evaluation.StructureTotals over several batches against a restatement
that never touches the device (tests/decode_ref.py decodes, tests/structure_ref.py counts, plain loops sum): the integers equal, the
float64 sums within 2^-52 times the sum of their (non-negative) terms, because torch's order of adding rows is not fixed;
sampling.run_generation / run_modification replaying recorded tokens with structure on and off - the same files, the same report, one
more launch per batch (modification: and one more decode and launch for the ground truth) and one more copy per run, none of either
when it is off; a sampler that returns the ground truth has no gap; a reference summary is carried into the report; one pass of each
of the three loops with the real sampler."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import structure_ref as sr  # noqa: E402
from musediffusion_amd import evaluation, metric, sampling  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402
from test_decode_cpu import fixture_cases  # noqa: E402
from test_evaluate_cpu import batches, fixture  # noqa: E402
from test_evaluate_gpu import _fatal, dev, fixture_loader, library_launches  # noqa: E402
from test_harmony_sampling_gpu import CopyCounter  # noqa: E402
from test_infill_sampling_gpu import KINDS, STEP, setup  # noqa: E402,F401
from test_pairstats_cpu import gen_batches  # noqa: E402

DEV = "cuda"
RATIOS = evaluation.StructureTotals.RATIO_NAMES
KERNEL = "structure_counts_kernel"


def host_counts(sc):
    return dict(counts=sc.counts.cpu().numpy(), entropy=sc.entropy.cpu().numpy(), status=sc.status.cpu().numpy(), bars=sc.bars.cpu().numpy())


def restate(batch_list, strict):
    """the vector of StructureTotals without the device: every row through the decode restatement with the product's capacities, the
    rows that decode through structure_ref.row_counts with StructureTotals' table size -> structure_ref.Totals"""
    totals = sr.Totals()
    for tokens, mask in batch_list:
        ld = min(2 * tokens.shape[1], dr.MAX_ROW)
        table = metric.xlog2x_host(ld // 4 + 1)
        for b in range(len(tokens)):
            r = dr.decode_row(tokens[b], mask[b], ld, ld // 4 + 1, ld // 2 + 1, strict)
            if r["status"] != dr.OK:
                continue
            counts, ent, _, st = sr.row_counts(r["notes"].tolist(), r["meta"], table, max_bars=min(512, ld + 1))
            assert st == sr.OK and counts[1] == 0
            totals.update(counts, ent)
    return totals


def same_vector(got, want):
    """got: StructureTotals.vector() on the host; want: a structure_ref.Totals"""
    w = want.vector()
    assert got[:12] == w[:12] and got[15] == w[15], (got, w)
    for i, terms in ((12, want.h1), (13, want.h4), (14, want.gs)):
        assert all(t >= 0 for t in terms) and abs(got[i] - w[i]) <= 2.0 ** -52 * math.fsum(terms), (i, got[i], w[i])


def same_summary(got, want):
    """two summaries of the same integers: equal fields, NaN where both are; the three means within 2^-52 relative twice over"""
    assert set(got) == set(want)
    for key, w in want.items():
        g = got[key]
        if key in ("h1", "h4", "gs"):
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 2.0 ** -51 * abs(w), (key, g, w)
        else:
            assert g == w or (math.isnan(g) and math.isnan(w)), (key, g, w)


# ------------------------------------------------------------------------------------------------ the fixture rows
def test_structure_counts_of_decoded_fixture_rows_equal_the_recorded_answers():
    checked = 0
    for c in fixture_cases():
        tokens, mask = dev(np.asarray(c.tokens)[None]), dev(np.asarray(c.mask)[None])
        for strict in (False, True):
            dec = du.decode_tokens(tokens, mask, strict_validation=strict)
            got = host_counts(metric.structure_counts(dec, max_bars=64, return_bars=True))
            if c.status[strict] != dr.OK:
                assert got["status"].tolist() == [sr.MASKED] and not any(got[k].any() for k in ("counts", "entropy", "bars")), c.name
                continue
            counts, ent, table, st = sr.row_counts(c.notes.tolist(), c.meta, metric.xlog2x_host(dec.notes.shape[1]), max_bars=64)
            assert got["status"].tolist() == [sr.OK] and got["counts"][0].tolist() == counts and got["bars"][0].tolist() == table, (c.name, strict)
            assert got["entropy"][0].view(np.int64).tolist() == np.array(ent, np.float64).view(np.int64).tolist(), (c.name, strict)
            assert counts[1] == 0 and counts[0] == len(c.notes)
            checked += 1
    assert checked > 60


# ------------------------------------------------------------------------------------------------ StructureTotals
def test_totals_over_several_batches():
    made = [dr.make_batch(seed, 320)[:2] for seed in (1, 2, 3)]
    for strict in (False, True):
        totals = evaluation.StructureTotals(DEV)
        for tokens, mask in made:
            assert totals.update(du.decode_tokens(dev(tokens), dev(mask), strict_validation=strict)) is totals
        vec = totals.vector()
        assert vec.dtype == torch.float64 and vec.shape == (16,) and vec.is_cuda
        want = restate(made, strict)
        same_vector(vec.cpu().tolist(), want)
        s = totals.summary()
        same_summary(s, evaluation.StructureTotals.ratios(want.vector()))
        assert s == totals.summary()                                    # the same call, the same bits
        assert s["rows"] > 90 and s["notes"] > 2000 and 1 < s["h1"] < s["h4"] < math.log2(12) and 0 < s["gs"] < 1 and 0 <= s["empty_bars"] < 0.5
        assert s["pitch_classes"] <= 12 and s["distinct_pitches"] <= s["pitch_range"] + 1 and s["onsets_per_bar"] <= s["notes_per_bar"]
    # nothing counted: NaN, not an error; a mask of the caller's
    empty = evaluation.StructureTotals(DEV).summary()
    assert empty["rows"] == 0 and all(math.isnan(empty[k]) for k in RATIOS)
    tokens, mask = made[0]
    dec = du.decode_tokens(dev(tokens), dev(mask))
    none = evaluation.StructureTotals(DEV).update(dec, valid=torch.zeros(len(tokens), device=DEV)).summary()
    assert none["rows"] == 0 and none["notes"] == 0 and math.isnan(none["h1"])
    half = evaluation.StructureTotals(DEV).update(dec, valid=dec.status.eq(du.OK) & (torch.arange(len(tokens), device=DEV) % 2 == 0)).summary()
    same_summary(half, evaluation.StructureTotals.ratios(restate([(tokens[::2], mask[::2])], False).vector()))


# ------------------------------------------------------------------------------------------------ the drivers
def test_run_generation_with_structure_writes_and_reports_what_the_run_without_it_does(tmp_path, monkeypatch):
    f = fixture()
    L = f["gen_tokens"].shape[1]
    copies = CopyCounter(monkeypatch)
    reps, logs, launches, n_copies = {}, {}, {}, {}
    for on in (False, True):
        trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
        logs[on] = []
        run = lambda: reps.update({on: sampling.run_generation(  # noqa: E731
            None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=6, out_dir=str(tmp_path / str(on)),
            sampler=lambda cond: next(trials), log=logs[on].append, get_metric=True, structure=on)})
        before = copies.n
        launches[on] = library_launches(run)
        n_copies[on] = copies.n - before
        logs[on] = [ln.replace(str(tmp_path / str(on)), "<out>") for ln in logs[on]]
    off, rep = reps[False], reps[True]
    assert (rep.total_valid_count, rep.batches, rep.summary) == (off.total_valid_count, off.batches, off.summary) and rep.batches == 2
    assert type(rep.totals) is type(off.totals) and rep.totals.summary() == off.totals.summary()
    names = sorted(os.listdir(tmp_path / "True"))
    assert names == sorted(os.listdir(tmp_path / "False")) == [str(x) for x in f["gen_names"][:7]]
    for name in names:
        assert open(tmp_path / "True" / name, "rb").read() == open(tmp_path / "False" / name, "rb").read()
    assert not hasattr(off, "structure") and [ln for ln in logs[True] if ln in logs[False]] == logs[False]
    assert set(rep.structure) == {"generated"}
    assert [ln for ln in logs[True] if ln not in logs[False]] == [evaluation.structure_block(rep.structure["generated"])]
    same_summary(rep.structure["generated"], evaluation.StructureTotals.ratios(restate(gen_batches()[:2], False).vector()))
    assert rep.structure["generated"]["rows"] == 7
    # one more launch per batch, one more copy per run; none of either without it
    kernel = [k for k in launches[True] if k.startswith(KERNEL)]
    assert len(kernel) == 2 and not [k for k in launches[False] if "structure" in k]
    assert sorted(k for k in launches[True] if k not in kernel) == sorted(launches[False])
    assert n_copies[True] == n_copies[False] + 1
    # a reference made beforehand is carried into the report, with the gap to it; without metrics the loop's own decode is the one counted
    reference = evaluation.StructureTotals(DEV).update(du.decode_tokens(*(dev(x) for x in dr.make_batch(4, 320)[:2]))).summary()
    trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
    log = []
    plain = sampling.run_generation(None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=100, out_dir=None, max_batches=3,
                                    sampler=lambda cond: next(trials), log=log.append, structure=True, structure_reference=reference)
    assert set(plain.structure) == {"generated", "reference", "gap"} and plain.structure["reference"] is reference
    same_summary(plain.structure["generated"], evaluation.StructureTotals.ratios(restate(gen_batches(), False).vector()))
    assert plain.structure["gap"] == evaluation.structure_gap(plain.structure["generated"], reference) and set(plain.structure["gap"]) == set(RATIOS)
    assert plain.totals is None and plain.structure["generated"]["rows"] == plain.total_valid_count == 14
    assert [evaluation.structure_block(plain.structure["generated"]), evaluation.structure_block(reference, "Structure of the reference"),
            evaluation.structure_block(plain.structure["gap"], "Structure gap")] == log[-3:]
    # no batch ran
    none = sampling.run_generation(None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=0, out_dir=None, log=lambda s: None,
                                   structure=True)
    assert none.structure is None and none.batches == 0


def test_run_modification_with_structure_writes_and_reports_what_the_run_without_it_does(tmp_path, monkeypatch):
    f, bs = fixture(), batches()
    copies = CopyCounter(monkeypatch)
    reps, logs, launches, n_copies = {}, {}, {}, {}
    for on, where in ((False, "a"), (True, "b"), (False, None), (True, None)):
        samples = iter([dev(b["sample"]) for b in bs])
        key = (on, where is not None)
        logs[key] = []
        run = lambda: reps.update({key: sampling.run_modification(  # noqa: E731
            None, None, fixture_loader(), step=100, batch_size=int(f["batch_size"]), out_dir=where and str(tmp_path / where),
            sampler=lambda cond: next(samples), log=logs[key].append, structure=on)})
        before = copies.n
        launches[key] = library_launches(run)
        n_copies[key] = copies.n - before
        if where:
            logs[key] = [ln.replace(str(tmp_path / where), "<out>") for ln in logs[key]]
    # with metrics the batch is decoded strictly, once; the ground truth is validated the same way
    want = evaluation.StructureTotals.ratios(restate([(b["sample"], b["mask"]) for b in bs], True).vector())
    want_ref = evaluation.StructureTotals.ratios(restate([(b["correct"], b["mask"]) for b in bs], True).vector())
    truth_decode = []
    for b in bs:
        truth_decode += library_launches(lambda: du.decode_tokens(dev(b["correct"]), dev(b["mask"]), strict_validation=True))
    for files in (True, False):
        off, rep = reps[(False, files)], reps[(True, files)]
        assert (rep.total_valid_count, rep.batches, rep.summary) == (off.total_valid_count, off.batches, off.summary) and rep.batches == 4
        assert rep.totals.vector().cpu().tolist() == off.totals.vector().cpu().tolist() and rep.total_valid_count == 38
        assert not hasattr(off, "structure") and [ln for ln in logs[(True, files)] if ln in logs[(False, files)]] == logs[(False, files)]
        s = rep.structure
        assert set(s) == {"generated", "reference", "gap"} and s["gap"] == evaluation.structure_gap(s["generated"], s["reference"])
        assert [ln for ln in logs[(True, files)] if ln not in logs[(False, files)]] == [
            evaluation.structure_block(s["generated"]), evaluation.structure_block(s["reference"], "Structure of the reference"),
            evaluation.structure_block(s["gap"], "Structure gap")]
        same_summary(s["generated"], want)
        same_summary(s["reference"], want_ref)
        assert s["generated"]["rows"] == 38 and s["reference"]["rows"] >= 38
        # two more launches per batch (the sample's and the ground truth's) and the ground truth's decode; one more copy per run
        kernel = [k for k in launches[(True, files)] if k.startswith(KERNEL)]
        assert len(kernel) == 8 and not [k for k in launches[(False, files)] if "structure" in k]
        assert sorted(k for k in launches[(True, files)] if k not in kernel) == sorted(launches[(False, files)] + truth_decode)
        assert n_copies[(True, files)] == n_copies[(False, files)] + 1
    assert n_copies[(False, False)] == 1, "without an output directory the run copies once"
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == sorted(str(x) for x in f["names"])
    for name in os.listdir(tmp_path / "a"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    # a sampler that returns the ground truth: no gap, in any field
    rep = sampling.run_modification(None, None, fixture_loader(), step=100, batch_size=int(f["batch_size"]), sampler=lambda cond: cond["correct_ids"].to(DEV),
                                    log=lambda s: None, structure=True)
    assert rep.structure["generated"] == rep.structure["reference"] and set(rep.structure["gap"]) == set(RATIOS)
    assert all(v == 0.0 for v in rep.structure["gap"].values()), rep.structure["gap"]
    # without ground truth in the batch there is no reference; without metrics the loop's own decode is the one counted
    samples = iter([dev(b["sample"]) for b in bs])
    loader = ({"input_ids": c["input_ids"], "input_mask": c["input_mask"]} for c in fixture_loader())
    rep = sampling.run_modification(None, None, loader, step=100, batch_size=int(f["batch_size"]), sampler=lambda cond: next(samples),
                                    log=lambda s: None, structure=True)
    assert set(rep.structure) == {"generated"} and rep.totals is None
    same_summary(rep.structure["generated"], evaluation.StructureTotals.ratios(restate([(b["sample"], b["mask"]) for b in bs], False).vector()))
    # a loader without a batch
    assert sampling.run_modification(None, None, [], step=100, batch_size=4, log=lambda s: None, structure=True).structure is None


def test_the_three_loops_with_structure_and_the_real_sampler(setup, monkeypatch, tmp_path):  # noqa: F811
    m, diff, cond, tokens, mask, noise, steps = setup
    diff.noise_fn, diff.rng_mode = None, "philox"
    torch.manual_seed(13)
    batch = {"input_ids": cond["input_ids"], "input_mask": cond["input_mask"], "correct_ids": cond["input_ids"]}
    piece = evaluation.StructureTotals.ratios(restate([(tokens, mask)], True).vector())
    # infill keeps the piece: the rows come back valid, and the reference is the piece itself
    seen = []
    real = sampling.infill
    monkeypatch.setattr(sampling, "infill", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    log = []
    rep = sampling.run_infill(m, diff, [batch], bars=(0, 1), step=STEP, room=1, batch_size=len(KINDS), log=log.append, structure=True)
    s = rep.structure
    assert len(seen) == 1 and set(s) == {"generated", "reference", "gap"} and rep.infill["rows"]["ok"] == 5
    same_summary(s["generated"], evaluation.StructureTotals.ratios(restate([(seen[0][0].cpu().numpy(), mask)], True).vector()))
    same_summary(s["reference"], piece)
    assert s["reference"]["rows"] == 4 and evaluation.structure_block(s["generated"]) in log and evaluation.structure_block(s["gap"], "Structure gap") in log
    assert not hasattr(sampling.run_infill(m, diff, [batch], bars=(0, 1), step=STEP, room=1, batch_size=len(KINDS), log=lambda s: None), "structure")
    # modify and generate return what the tiny model makes of noise: mostly invalid rows, and a row on which the decode raises makes
    # the loop raise as it does without the keyword (tests/test_evaluate_gpu.py)
    for name in ("modify", "generate"):
        real_fn = getattr(sampling, name)
        monkeypatch.setattr(sampling, name, lambda *a, _real=real_fn, **k: seen.append(_real(*a, **k)) or seen[-1])
    del seen[:]
    try:
        rep = sampling.run_modification(m, diff, [batch], step=STEP, batch_size=len(KINDS), log=lambda s: None, structure=True)
    except (IndexError, KeyError, RuntimeError):
        rep = None
    assert len(seen) == 1
    if _fatal(seen[0], dev(mask), True):
        assert rep is None
    else:
        same_summary(rep.structure["generated"], evaluation.StructureTotals.ratios(restate([(seen[0].cpu().numpy(), mask)], True).vector()))
        same_summary(rep.structure["reference"], piece)
    del seen[:]
    meta = tokens[0, :11].tolist()
    L = tokens.shape[1]
    try:
        rep = sampling.run_generation(m, diff, meta, batch_size=len(KINDS), seq_len=L, num_samples=1000, step=STEP, out_dir=None, max_batches=1,
                                      log=lambda s: None, structure=True, structure_reference=piece)
    except (IndexError, KeyError, RuntimeError):
        rep = None
    assert len(seen) == 1
    gen_mask = du.meta_to_batch(meta, len(KINDS), L)["input_mask"]
    if _fatal(seen[0], gen_mask, False):
        assert rep is None
    else:
        same_summary(rep.structure["generated"], evaluation.StructureTotals.ratios(restate([(seen[0].cpu().numpy(), gen_mask.cpu().numpy())], False).vector()))
        assert rep.structure["reference"] is piece and set(rep.structure["gap"]) == set(RATIOS)
