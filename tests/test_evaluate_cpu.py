"""CPU: the evaluation end of the sampling run without a device.  tests/evaluate_ref.py (the numpy restatement of the fused
nearest-neighbour kernel and of evaluate_batch / MetricTotals) against every record of tests/golden/evaluate.npz - what the reference's
own decode_batch, ONNC, Controllability_* and the block run/sample.py:245-273 answered (tools/make_golden_evaluate.py); the fp32
operation order against float64 and the bound the GPU tests judge the kernel by; the driver loops of musediffusion_amd.sampling with an
injected sampler and a stub decode.  No kernel runs here: the device side is tests/test_evaluate_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import evaluate_ref as ev
from musediffusion_amd import _lib, evaluation, sampling
from musediffusion_amd.utils import decode_util as du

FIX = {}


def fixture():
    if not FIX:
        FIX.update(load_golden("evaluate.npz"))
    return FIX


def batches():
    """-> per batch dict(sample, correct, mask, valid, and the reference's records)"""
    f = fixture()
    out = []
    for n in range(len(f["valid_count"])):
        lo, hi = f["batch_off"][n], f["batch_off"][n + 1]
        mlo, mhi = f["most_off"][n], f["most_off"][n + 1]
        out.append(dict(sample=f["sample"][lo:hi], correct=f["correct"][lo:hi], mask=f["mask"][lo:hi], valid=~f["invalid"][lo:hi],
                        valid_count=int(f["valid_count"][n]), onnc=f["onnc"][n], cp=tuple(f["cp"][n]), cv=tuple(f["cv"][n]),
                        totals=f["totals"][n], most=f["most"][mlo:mhi], vec=f["vec"][mlo:mhi],
                        names=list(f["names"][f["names_off"][n]:f["names_off"][n + 1]]), printed=str(f["printed"][n])))
    return out


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_shape():
    """four batches of 8 to 24 rows, one without a valid row, one whose first ground-truth row has a NaN harmony vector"""
    bs = batches()
    assert [len(b["sample"]) for b in bs] == [8, 24, 12, 16] and os.path.getsize(os.path.join(GOLDEN, "evaluate.npz")) < 128 << 10
    assert [b["valid_count"] for b in bs].count(0) == 1 and all(0 < b["valid_count"] < len(b["sample"]) for b in bs if b["valid_count"])
    nan_batches = [n for n, b in enumerate(bs) if np.isnan(b["vec"]).any()]
    assert nan_batches == [3] and np.isnan(bs[3]["vec"][0, 44:]).all() and not np.isnan(bs[3]["vec"][1:]).any()


def test_restatement_reproduces_every_record():
    totals = ev.Totals()
    for n, b in enumerate(batches()):
        m = ev.evaluate_batch(b["sample"], b["correct"], b["mask"])
        assert np.array_equal(m["valid"], b["valid"]) and m["valid_count"] == b["valid_count"] and m["fatal"] == 0, n
        totals.update(m)
        if b["valid_count"]:
            both = np.concatenate([b["valid"], b["valid"]])
            assert np.allclose(m["vec"][both], b["vec"], rtol=1e-5, atol=1e-12, equal_nan=True), n
            assert np.array_equal(m["most"], ev.uncompact(b["most"], b["valid"])), n
            assert m["onnc"] == b["onnc"] and m["counts"] == b["cp"] + b["cv"], (n, m["onnc"], m["counts"])
        else:
            assert np.isnan(m["onnc"]) and m["counts"] == (0, 0, 0, 0) and (m["most"] == -1).all()
            assert np.array_equal(totals.vector(), before), "a batch without a valid row leaves the totals unchanged"
        before = totals.vector()
        assert before[1:] == [int(x) for x in b["totals"][1:]], (n, before, b["totals"])
        assert abs(before[0] - b["totals"][0]) <= (n + 1) * 2.0 ** -23 * abs(b["totals"][0]), (n, before[0], b["totals"][0])
    s, ref = totals.summary(), fixture()["summary"]
    # the reference divides fp32 tensors, the summary here Python floats: the ratios of equal integers agree to an fp32 rounding
    assert abs(s["onnc"] - ref[0]) <= 5 * 2.0 ** -23 * ref[0] and s["valid"] == 38
    assert abs(s["cp"] - ref[1]) <= 2.0 ** -24 * ref[1] and abs(s["cv"] - ref[2]) <= 2.0 ** -24 * ref[2]


def test_fixture_condition_best_exceeds_second_best():
    """in float64 every row without a NaN similarity has best > second best by a relative 1e-4: the fp32 orders of the reference's
    GEMMs, of the GEMM path here and of the fused kernel cannot disagree on these batches"""
    checked = 0
    for b in batches():
        if not b["valid_count"]:
            continue
        s = ev.sim64(b["vec"], b["vec"])
        np.fill_diagonal(s, 0.0)
        for i in range(len(s)):
            if np.isnan(s[i]).any():
                continue
            top = np.sort(s[i])[::-1]
            assert top[0] > 0 and top[0] - top[1] > 1e-4 * top[0], (i, top[:2])
            checked += 1
    assert checked == 2 * (6 + 19)


# ------------------------------------------------------------------------------------------------------------------ the bound
def _worst(q, k, inject=None, rows=512):
    """max over pairs of |sim32 - sim64| / bound (finite pairs with a nonzero bound), and where"""
    worst, where = 0.0, None
    for lo in range(0, len(q), rows):
        inj = (inject[0] - lo, inject[1], inject[2]) if inject and lo <= inject[0] < lo + rows else None
        s32 = ev.sim32(q[lo:lo + rows], k, inj).astype(np.float64)
        s64, bd = ev.sim64(q[lo:lo + rows], k), ev.bound(q[lo:lo + rows], k)
        ok = np.isfinite(s64) & (bd > 0)
        assert np.array_equal(np.isnan(s32), np.isnan(s64)) and (s32[np.isfinite(s64) & (bd == 0)] == 0).all()
        ratio = np.where(ok, np.abs(s32 - s64) / np.where(ok, bd, 1), 0)
        if ratio.max() > worst:
            i, j = np.unravel_index(ratio.argmax(), ratio.shape)
            worst, where = float(ratio.max()), (lo + int(i), int(j))
    return worst, where


def test_fp32_order_stays_within_half_the_bound_on_the_fixture():
    for b in batches():
        if b["valid_count"]:
            assert _worst(b["vec"], b["vec"])[0] <= 0.5


def test_fp32_order_stays_within_half_the_bound_on_random_unit_vectors():
    v = ev.unit_vectors(np.random.default_rng(5), 4096)
    s = ev.sim64(v[:64], v)
    assert ((s == 0) | (s >= 1e-20)).all() and (s == 0).any()
    worst, _ = _worst(v, v)
    assert 0 < worst <= 0.5, worst
    i, j = 1234, int(np.flatnonzero(ev.sim64(v[1234:1235], v)[0] > 0)[7])
    worst, where = _worst(v, v, inject=(i, j, 4 * ev.TAU))                 # the control: one pair off by 4 tau
    assert worst > 1 and where == (i, j), (worst, where)


def test_selection_rule_and_acceptance_rule():
    nan = np.float32("nan")
    sim = np.array([[1, 3, 3, 2], [0, 0, 0, 0], [1, nan, 5, nan], [nan, 1, 2, 3], [-0.0, 0.0, 0, -0.0]], np.float32)
    most, best = ev.select(sim)
    assert most.tolist() == [1, 0, 1, 0, 0] and best[0] == 3 and best[1] == 0 and np.isnan(best[2])
    most, best = ev.select(sim, q_valid=[1, 0, 1, 1, 1], k_valid=[0, 0, 1, 1])
    assert most.tolist() == [2, -1, 3, 3, 2] and best.tolist()[:2] == [3, 0] and np.isnan(best[2])
    assert (ev.select(sim, k_valid=[0, 0, 0, 0])[0] == -1).all()
    s64 = sim.astype(np.float64)
    assert not ev.accepted(s64, [1, 0, 1, 0, 0]) and not ev.accepted(s64, [2, 3, 1, 0, 1])     # ties within (1 - 2 tau): either index
    assert [r for r, _, _ in ev.accepted(s64, [0, 0, 3, 1, 2])] == [0, 2, 3]
    assert [r for r, _, _ in ev.accepted(s64, [2, 0, 3, 3, 2], q_valid=[1, 0, 1, 1, 1], k_valid=[0, 0, 1, 1])] == [1]
    assert ev.uncompact([2, 0, 1, 3], [False, True, True]).tolist() == [-1, 4, 1, -1, 2, 5]


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    L = _lib.lib()
    buf = (C.c_float * 112)()
    most = (C.c_int32 * 2)()
    a, m = C.addressof(buf), C.addressof(most)
    for args in ((None, 2, a, 2, None, None, 0, m), (a, 0, a, 2, None, None, 0, m), (a, 2, a, 0, None, None, 0, m),
                 (a, 2, a, 1 << 26, None, None, 0, m), (a, 2, a, 2, None, None, 0, None), (a, 2, a + 224, 1, None, None, 1, m),
                 (a, 2, a, 1, None, None, 1, m), (a, 2, a, 2, m, None, 1, m), (a, 2, a, 2, None, None, 2, m)):
        assert L.mhe_msim_nearest(*args, None, None, None) == _lib.MH_ERR_INVALID, args
        assert b"msim_nearest" in L.mh_last_error()


# ------------------------------------------------------------------------------------------------------------------ the driver
META = [580, 610, 627, 633, 639, 644, 651, 660, 700, 720, 727]


class StubDecoded:
    """what the driver uses of a DecodedBatch: .status on the tokens' device and .cpu() -> DecodedRows"""

    def __init__(self, status):
        self.status = status

    def cpu(self):
        st = self.status.numpy()
        B = len(st)
        notes = [np.array([[0, 480, 60, 100]], np.int32) if s == du.OK else np.zeros((0, 4), np.int32) for s in st]
        return du.DecodedRows(st, np.tile(np.array(META, np.int32), (B, 1)), np.zeros((B, 3), np.int32), notes,
                              [np.zeros((0, 2), np.int32)] * B)


@pytest.fixture
def stub(monkeypatch):
    """decode: the row's status is its first token; evaluate: onnc = the share of valid rows, CP (valid, 1), CV (10 valid, valid)"""
    calls = {"decode": [], "evaluate": 0}

    def decode_tokens(tokens, mask, strict_validation=False, **kw):
        calls["decode"].append(bool(strict_validation))
        return StubDecoded(tokens[:, 0].to(torch.int32))

    def evaluate_batch(tokens, correct_ids, mask, strict_validation=True):
        calls["evaluate"] += 1
        dec = decode_tokens(tokens, mask, strict_validation)
        valid = dec.status == du.OK
        n = valid.sum()
        counts = torch.stack([n, torch.ones_like(n), 10 * n, n])
        return evaluation.BatchMetrics(valid, n, (n / len(valid)).float() / (n > 0), counts, None, torch.zeros((), dtype=torch.int32), dec)

    monkeypatch.setattr(du, "decode_tokens", decode_tokens)
    monkeypatch.setattr(evaluation, "evaluate_batch", evaluate_batch)
    monkeypatch.setattr(du, "meta_to_batch", lambda meta, B, L, device="cuda": {"input_ids": torch.zeros(B, L, dtype=torch.int32),
                                                                             "input_mask": torch.ones(B, L, dtype=torch.int32)})
    return calls


def _rows(statuses):
    t = torch.zeros(len(statuses), 6, dtype=torch.int64)
    t[:, 0] = torch.tensor(statuses)
    return t


def _loader(status_batches, correct=True):
    for st in status_batches:
        t = _rows(st)
        yield {"input_ids": t, "input_mask": torch.ones_like(t), **({"correct_ids": t} if correct else {})}


MOD = [[du.OK, du.NO_EOS, du.OK, du.OK], [du.STRICT_FAILED] * 4, [du.OK, du.ONCE_FAILED, du.RESTORE_FAILED]]


def test_run_modification_names_numbers_and_reports(stub, tmp_path):
    log = []
    rep = sampling.run_modification(None, None, _loader(MOD), step=10, batch_size=4, out_dir=str(tmp_path / "out"), log=log.append,
                                    sampler=lambda cond: cond["input_ids"])
    assert sorted(os.listdir(tmp_path / "out")) == ["0000000_batch00000_0000.midi", "0000002_batch00000_0002.midi",
                                                    "0000003_batch00000_0003.midi", "0000008_batch00002_0000.midi"]
    assert du.read_midi(tmp_path / "out" / "0000008_batch00002_0000.midi")[1].tolist() == [[0, 480, 60, 100]]
    assert rep.total_valid_count == 4 and rep.batches == 3 and stub["decode"] == [True] * 3 and stub["evaluate"] == 3
    # onnc_sum = 3 * 0.75 + 1 * (1 / 3); the batch without a valid row (0 / 0) adds nothing
    want = {"onnc": float(np.float32(2.25) + np.float32(1) * (np.float32(1) / np.float32(3))) / 4, "cp": 3 / 4, "cv": 4 / 40, "valid": 4.0}
    assert rep.summary == pytest.approx(want, rel=1e-6) and rep.totals.summary() == rep.summary
    text = "\n".join(log)
    assert text.count(" Metric of Batch ") == 2 and "Metric of Batch 1" not in text
    assert "=================== Metric of Batch 0 ====================" in text
    assert "                       ONNC: 0.750000                       " in text
    assert "                        CP: 0.333333                        " in text
    assert " * Index (in batch 0) of invalid sequence:\n    [1]" in text and " * 4 sequences are invalid." in text
    assert text.index("Summary of Batch 2") < text.index("Metric of Batch 2") < text.index(" Summary: Metric ")
    assert evaluation.summary_block(rep.summary) in log
    assert log[-2].splitlines()[1:] == ["===================== Summary: Metric ======================",
                                       "                       ONNC: %.6f                       " % want["onnc"],
                                       "                        CP: 0.750000                        ",
                                       "                        CV: 0.100000                        ", "=" * 60]
    # without an output directory: the same totals, the blocks from one copy at the end, nothing written
    log2 = []
    rep2 = sampling.run_modification(None, None, _loader(MOD), step=10, batch_size=4, log=log2.append, sampler=lambda cond: cond["input_ids"])
    assert rep2.summary == rep.summary and rep2.total_valid_count == 4 and rep2.totals.vector().tolist() == rep.totals.vector().tolist()
    assert [ln for ln in log2 if "Metric" in ln] == [ln for ln in log if "Metric" in ln and "Summary of Batch" not in ln]
    # without ground truth, or with get_metric off: the plain decode (not strict), counts only
    del stub["decode"][:]
    rep3 = sampling.run_modification(None, None, _loader(MOD, correct=False), step=10, batch_size=4, log=log2.append,
                                     sampler=lambda cond: cond["input_ids"])
    rep4 = sampling.run_modification(None, None, _loader(MOD), step=10, batch_size=4, get_metric=False, log=log2.append,
                                     sampler=lambda cond: cond["input_ids"])
    assert rep3.total_valid_count == rep4.total_valid_count == 4 and rep3.totals is rep4.totals is rep3.summary is None
    assert stub["decode"] == [False] * 6 and stub["evaluate"] == 6


def test_run_modification_raises_where_write_decoded_rows_does(stub, tmp_path):
    bad = [[du.OK, du.BAD_META]]
    with pytest.raises(KeyError):
        sampling.run_modification(None, None, _loader(bad), step=10, batch_size=2, out_dir=str(tmp_path), log=lambda s: None,
                                  sampler=lambda cond: cond["input_ids"])
    totals = evaluation.MetricTotals("cpu")
    totals.fatal = torch.tensor(du.REF_INDEXERROR, dtype=torch.int32)
    with pytest.raises(IndexError):
        totals.summary()


def test_run_generation_numbering_stop_and_max_batches(stub, tmp_path):
    trials = iter([[du.NO_EOS] * 4, [du.OK, du.NO_EOS, du.OK, du.ONCE_FAILED], [du.OK] * 4, [du.OK] * 4])
    log = []
    rep = sampling.run_generation(None, None, META, batch_size=4, seq_len=6, num_samples=5, out_dir=str(tmp_path / "gen"), log=log.append,
                                  sampler=lambda cond: _rows(next(trials)))
    # 0 + 2 + 4 = 6 >= 5: the loop stops after the third batch, having written one file more than asked for
    assert rep.total_valid_count == 6 and rep.batches == 3 and next(trials) == [du.OK] * 4
    assert sorted(os.listdir(tmp_path / "gen")) == ["generated_%07d.midi" % n for n in range(6)]
    text = "\n".join(log)
    assert "Summary of Trial 1" in text and " * Totally 2 sequences are converted." in text and " * Totally 6 sequences are converted." in text
    assert stub["decode"] == [False] * 3
    rep = sampling.run_generation(None, None, META, batch_size=4, seq_len=6, num_samples=5, out_dir=str(tmp_path / "none"), max_batches=7,
                                  log=log.append, sampler=lambda cond: _rows([du.NO_EOS] * 4))
    assert rep.total_valid_count == 0 and rep.batches == 7 and os.listdir(tmp_path / "none") == []
