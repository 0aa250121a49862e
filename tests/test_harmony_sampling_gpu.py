"""GPU: the chord-fit counts above the kernel.  metric.harmony_counts on decode_tokens of every record of tests/golden/decode.npz
against the restatement on the reference's own recorded notes and markers; Controllability_Harmony; evaluation.HarmonyTotals over
several batches, with and without a bar range, against a restatement that never touches the device (tests/decode_ref.py decodes,
tests/harmony_ref.py counts, plain loops sum); sampling.run_generation / run_modification replaying recorded tokens with harmony on
and off - the same files, the same report, one more launch per batch and one more copy per run, and none of either when it is off;
one pass of run_infill with the real sampler, whose regenerated and kept bars must add up to the piece."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import harmony_ref as hr  # noqa: E402
import infill_ref as ir  # noqa: E402
from musediffusion_amd import evaluation, metric, sampling  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402
from test_decode_cpu import fixture_cases  # noqa: E402
from test_evaluate_cpu import batches, fixture  # noqa: E402
from test_evaluate_gpu import dev, fixture_loader, library_launches  # noqa: E402
from test_harmony_cpu import CHORD, first_bar_shift  # noqa: E402
from test_infill_sampling_gpu import KINDS, STEP, setup  # noqa: E402,F401
from test_pairstats_cpu import gen_batches  # noqa: E402

DEV = "cuda"
TABLE = 64          # bars of the restatement's per-bar table: more than any piece here has


def host_counts(hc):
    return dict(counts=hc.counts.cpu().numpy(), status=hc.status.cpu().numpy(), hist=hc.hist.cpu().numpy(), bars=hc.bars.cpu().numpy())


def restate(batch_list, strict, bars=None):
    """the totals of HarmonyTotals without the device: every row through the decode restatement with the product's capacities, the
    rows that decode through harmony_ref.row_counts, summed in Python -> harmony_ref.summary's dict plus 'rows'"""
    counts, hist, region, rows = [0] * 8, [0] * 12, [0, 0], 0
    for n, (tokens, mask) in enumerate(batch_list):
        ld = min(2 * tokens.shape[1], dr.MAX_ROW)
        for b in range(len(tokens)):
            r = dr.decode_row(tokens[b], mask[b], ld, ld // 4 + 1, ld // 2 + 1, strict)
            if r["status"] != dr.OK:
                continue
            c, h, table, st = hr.row_counts(r["notes"].tolist(), r["chords"].tolist(), r["meta"], max_bars=TABLE)
            assert st == hr.OK and c[7] <= TABLE
            rows += 1
            counts = [x + y for x, y in zip(counts, c)]
            hist = [x + y for x, y in zip(hist, h)]
            if bars is not None:
                lo, hi = bars if isinstance(bars, tuple) else (int(x) for x in bars[n][b])
                shift = first_bar_shift(r["restored"])
                for k in range(max(lo + shift, 0), min(hi + shift, TABLE)):
                    region[0] += table[k][1]
                    region[1] += table[k][2]
    rest = [counts[1] - region[0], counts[2] - region[1]]
    out = hr.summary(counts, hist, *((region, rest) if bars is not None else ()))
    out["rows"] = rows
    return out


def same_summary(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        if key == "pitch_class_entropy":                               # a dozen double operations on exact integers
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-12 * abs(w), (key, g, w)
        else:                                                          # integers, and ratios of equal integers: the same division
            assert g == w or (isinstance(w, float) and math.isnan(g) and math.isnan(w)), (key, g, w)


# ------------------------------------------------------------------------------------------------ the fixture rows
def test_harmony_counts_of_decoded_fixture_rows_equal_the_recorded_answers():
    checked = 0
    for c in fixture_cases():
        tokens, mask = dev(np.asarray(c.tokens)[None]), dev(np.asarray(c.mask)[None])
        for strict in (False, True):
            dec = du.decode_tokens(tokens, mask, strict_validation=strict)
            got = host_counts(metric.harmony_counts(dec, max_bars=TABLE, return_hist=True))
            if c.status[strict] != dr.OK:
                assert got["status"].tolist() == [hr.MASKED] and not any(got[k].any() for k in ("counts", "hist", "bars")), c.name
                continue
            recorded = [(int(t), CHORD(name)) for t, name in zip(c.marker_time, c.marker_text)]
            counts, hist, table, st = hr.row_counts(c.notes.tolist(), recorded, c.meta, max_bars=TABLE)
            assert got["status"].tolist() == [hr.OK] and got["counts"][0].tolist() == counts and got["hist"][0].tolist() == hist, (c.name, strict)
            assert got["bars"][0].tolist() == table, (c.name, strict)
            total, wrong = metric.Controllability_Harmony(dec)
            assert (total, wrong) == (counts[1], counts[1] - counts[2]) and isinstance(total, int) and isinstance(wrong, int)
            checked += 1
    assert checked > 60


def test_controllability_harmony_is_the_sum_over_the_valid_rows():
    tokens, mask, _ = dr.make_batch(5, 320)
    dec = du.decode_tokens(dev(tokens), dev(mask))
    want = restate([(tokens, mask)], False)
    assert metric.Controllability_Harmony(dec) == (want["judged"], round(want["ch"] * want["judged"])) and want["judged"] > 500
    every_other = torch.arange(len(tokens), device=DEV) % 2 == 0
    half = restate([(tokens[::2], mask[::2])], False)
    assert metric.Controllability_Harmony(dec, dec.status.eq(du.OK) & every_other)[0] == half["judged"] < want["judged"]
    hc = metric.harmony_counts(dec)
    assert hc.bars is None and hc.hist is None and hc.status.eq(hr.MASKED).sum() == dec.status.ne(du.OK).sum()


# ------------------------------------------------------------------------------------------------ HarmonyTotals
def test_totals_over_several_batches_with_and_without_bars():
    made = [dr.make_batch(seed, 320)[:2] for seed in (1, 2, 3)]
    g = np.random.default_rng(8)
    per_row = [np.stack([np.array(sorted(g.choice(np.arange(0, 9), size=2, replace=False))) for _ in range(len(t))]) for t, _ in made]
    for strict in (False, True):
        for bars in (None, (1, 3), (0, 1), per_row):
            totals = evaluation.HarmonyTotals(DEV)
            for n, (tokens, mask) in enumerate(made):
                dec = du.decode_tokens(dev(tokens), dev(mask), strict_validation=strict)
                b = bars if bars is None or isinstance(bars, tuple) else (torch.from_numpy(bars[n]) if n % 2 else dev(bars[n]))
                assert totals.update(dec, bars=b) is totals
            s = totals.summary()
            want = restate(made, strict, bars)
            same_summary(s, want)
            same_summary(totals.summary(), s)                          # the same call, the same bits
            assert s["rows"] > 90 and s["judged"] > 2000 and 0 < s["ch"] < 1 and 0 < s["out_of_scale"] < 1 and 3 < s["pitch_class_entropy"] <= math.log2(12)
            if bars is not None:
                assert s["judged_region"] + s["judged_rest"] == s["judged"] and 0 < s["judged_region"] < s["judged"]
                assert evaluation.harmony_block(s).count("CH") == 4
    # nothing counted: NaN, not an error; a mask of the caller's
    empty = evaluation.HarmonyTotals(DEV).summary()
    assert empty["rows"] == 0 and all(math.isnan(empty[k]) for k in ("ch", "ch_ticks", "out_of_scale", "judged_share", "pitch_class_entropy"))
    tokens, mask = made[0]
    dec = du.decode_tokens(dev(tokens), dev(mask))
    none = evaluation.HarmonyTotals(DEV).update(dec, valid=torch.zeros(len(tokens), device=DEV), bars=(0, 2)).summary()
    assert none["rows"] == 0 and math.isnan(none["ch_region"]) and math.isnan(none["ch_rest"]) and none["judged_region"] == 0
    with pytest.raises(ValueError):
        evaluation.HarmonyTotals(DEV).update(dec, bars=torch.zeros(3, 2))


# ------------------------------------------------------------------------------------------------ the drivers
class CopyCounter:
    """counts the device -> host copies made through Tensor.cpu / Tensor.tolist / Tensor.item of device tensors"""

    def __init__(self, monkeypatch):
        self.n = 0
        for name in ("cpu", "item"):
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, self.wrap(real))

    def wrap(self, real):
        def counted(t, *a, **k):
            self.n += bool(t.is_cuda)
            return real(t, *a, **k)
        return counted


def test_run_generation_with_harmony_writes_and_reports_what_the_run_without_it_does(tmp_path, monkeypatch):
    f = fixture()
    L = f["gen_tokens"].shape[1]
    copies = CopyCounter(monkeypatch)
    reps, logs, launches, n_copies = {}, {}, {}, {}
    for on in (False, True):
        trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
        logs[on] = []
        run = lambda: reps.update({on: sampling.run_generation(  # noqa: E731
            None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=6, out_dir=str(tmp_path / str(on)),
            sampler=lambda cond: next(trials), log=logs[on].append, get_metric=True, harmony=on)})
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
    assert not hasattr(off, "harmony") and [ln for ln in logs[True] if ln in logs[False]] == logs[False]
    assert [ln for ln in logs[True] if ln not in logs[False]] == [evaluation.harmony_block(rep.harmony)]
    same_summary(rep.harmony, restate(gen_batches()[:2], False))
    assert rep.harmony["rows"] == 7
    # one more launch per batch, one more copy per run; none of either without it
    kernel = [k for k in launches[True] if k.startswith("harmony_counts_kernel")]
    assert len(kernel) == 2 and not [k for k in launches[False] if "harmony" in k]
    assert sorted(k for k in launches[True] if k not in kernel) == sorted(launches[False])
    assert n_copies[True] == n_copies[False] + 1
    # without metrics the loop's own decode is the one that is judged
    trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
    plain = sampling.run_generation(None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=L, num_samples=100, out_dir=None, max_batches=3,
                                    sampler=lambda cond: next(trials), log=lambda s: None, harmony=True)
    same_summary(plain.harmony, restate(gen_batches(), False))
    assert plain.totals is None and plain.harmony["rows"] == plain.total_valid_count == 14


def test_run_modification_with_harmony_writes_and_reports_what_the_run_without_it_does(tmp_path, monkeypatch):
    f, bs = fixture(), batches()
    copies = CopyCounter(monkeypatch)
    reps, logs, launches, n_copies = {}, {}, {}, {}
    for on, where in ((False, "a"), (True, "b"), (False, None), (True, None)):
        samples = iter([dev(b["sample"]) for b in bs])
        key = (on, where is not None)
        logs[key] = []
        run = lambda: reps.update({key: sampling.run_modification(  # noqa: E731
            None, None, fixture_loader(), step=100, batch_size=int(f["batch_size"]), out_dir=where and str(tmp_path / where),
            sampler=lambda cond: next(samples), log=logs[key].append, harmony=on)})
        before = copies.n
        launches[key] = library_launches(run)
        n_copies[key] = copies.n - before
        if where:
            logs[key] = [ln.replace(str(tmp_path / where), "<out>") for ln in logs[key]]
    want = restate([(b["sample"], b["mask"]) for b in bs], True)       # with metrics the batch is decoded strictly, once
    for files in (True, False):
        off, rep = reps[(False, files)], reps[(True, files)]
        assert (rep.total_valid_count, rep.batches, rep.summary) == (off.total_valid_count, off.batches, off.summary) and rep.batches == 4
        assert rep.totals.vector().cpu().tolist() == off.totals.vector().cpu().tolist() and rep.total_valid_count == 38
        assert not hasattr(off, "harmony") and [ln for ln in logs[(True, files)] if ln in logs[(False, files)]] == logs[(False, files)]
        assert [ln for ln in logs[(True, files)] if ln not in logs[(False, files)]] == [evaluation.harmony_block(rep.harmony)]
        same_summary(rep.harmony, want)
        assert rep.harmony["rows"] == 38
        kernel = [k for k in launches[(True, files)] if k.startswith("harmony_counts_kernel")]
        assert len(kernel) == 4 and not [k for k in launches[(False, files)] if "harmony" in k]
        assert sorted(k for k in launches[(True, files)] if k not in kernel) == sorted(launches[(False, files)])
        assert n_copies[(True, files)] == n_copies[(False, files)] + 1
    assert n_copies[(False, False)] == 1, "without an output directory the run copies once"
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == sorted(str(x) for x in f["names"])
    for name in os.listdir(tmp_path / "a"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    # a restriction to bars, as run_infill passes it
    samples = iter([dev(b["sample"]) for b in bs])
    rep = sampling.run_modification(None, None, fixture_loader(), step=100, batch_size=int(f["batch_size"]), sampler=lambda cond: next(samples),
                                    log=lambda s: None, harmony=True, harmony_bars=(1, 2))
    same_summary(rep.harmony, restate([(b["sample"], b["mask"]) for b in bs], True, (1, 2)))
    # a loader without a batch
    assert sampling.run_modification(None, None, [], step=100, batch_size=4, log=lambda s: None, harmony=True).harmony is None


def test_run_infill_with_harmony_and_the_real_sampler(setup, monkeypatch):  # noqa: F811
    m, diff, cond, tokens, mask, noise, steps = setup
    diff.noise_fn, diff.rng_mode = None, "philox"
    batch = {"input_ids": cond["input_ids"], "input_mask": cond["input_mask"], "correct_ids": cond["input_ids"]}
    seen = []
    real = sampling.infill
    monkeypatch.setattr(sampling, "infill", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    log = []
    rep = sampling.run_infill(m, diff, [batch], bars=(0, 1), step=STEP, room=1, batch_size=len(KINDS), log=log.append, harmony=True)
    s = rep.harmony
    assert "ch_region" in s and "ch_rest" in s and s["judged_region"] + s["judged_rest"] == s["judged"]
    assert rep.infill["rows"]["ok"] == 5 and evaluation.harmony_block(s) in log
    assert len(seen) == 1
    same_summary(s, restate([(seen[0][0].cpu().numpy(), mask)], True, (0, 1)))
    # the piece itself, judged the same way: the kept bars are the piece's, so they fit their chords as they did
    piece = evaluation.HarmonyTotals(DEV).update(du.decode_tokens(dev(tokens), dev(mask), strict_validation=True), bars=(0, 1)).summary()
    same_summary(piece, restate([(tokens, mask)], True, (0, 1)))
    assert piece["judged_rest"] > 0 and (s["rows"] < piece["rows"] or s["judged_rest"] == piece["judged_rest"])
    assert ir.OK == 0
