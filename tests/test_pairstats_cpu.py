"""CPU: the pair statistics of a set without a device.  tests/pairstats_ref.py (the numpy restatement of csrc/pairstats.hip's rules and
of evaluation.GenerationTotals) on hand-made sets; the float64 accumulation bound the GPU tests judge sum[i] by, against math.fsum; the
self-similarity check behind the default duplicate threshold;
the refusals of mhs_msim_pair_stats, which come before any launch; sampling.run_generation(get_metric=True) with a stub decode and the
restatement standing in for the kernels.  No kernel runs here: the device side is tests/test_pairstats_gpu.py and
tests/test_generation_metrics_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import evaluate_ref as ev
import pairstats_ref as pr
from musediffusion_amd import _lib, evaluation, metric, sampling
from musediffusion_amd.utils import decode_util as du
from test_evaluate_cpu import META, StubDecoded, _rows, fixture

NAN = np.float32("nan")


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_rules_on_a_three_row_set():
    sim = np.array([[9, 0.5, 0.25], [0.5, 9, 0.125], [0.25, 0.125, 9]], np.float32)     # the diagonal (9) must touch nothing
    on = pr.counted(3, 3, self_mode=True)
    assert on.tolist() == [[False, True, True], [True, False, True], [True, True, False]]
    total, count, nan, above = pr.reduce_rows(sim, on, 0.25)
    assert total.tolist() == [0.75, 0.625, 0.375] and count.tolist() == [2, 2, 2] and nan.tolist() == [0, 0, 0]
    assert above.tolist() == [2, 1, 1]                                                   # >=, not >: 0.25 itself counts
    assert pr.reduce_rows(sim, on, np.nextafter(np.float32(0.25), np.float32(1)))[3].tolist() == [1, 1, 0]
    assert pr.reduce_rows(sim, on, float("nan"))[3].tolist() == [0, 0, 0] and pr.reduce_rows(sim, on)[3] is None
    # two-set mode: the diagonal is a pair like any other
    total, count, _, _ = pr.reduce_rows(sim, pr.counted(3, 3), 0.0)
    assert total.tolist() == [9.75, 9.625, 9.375] and count.tolist() == [3, 3, 3]
    # a masked row is neither a query (zeros) nor a key
    total, count, nan, above = pr.reduce_rows(sim, pr.counted(3, 3, [1, 0, 1], [1, 0, 1], self_mode=True), 0.0)
    assert total.tolist() == [0.25, 0.0, 0.25] and count.tolist() == [1, 0, 1] and above.tolist() == [1, 0, 1] and nan.tolist() == [0, 0, 0]


def test_rules_on_a_four_row_set_with_a_nan_row_a_masked_row_and_groups():
    sim = np.array([[1, 0.5, NAN, 0.25], [0.5, 1, NAN, 0], [NAN, NAN, NAN, NAN], [0.25, 0, NAN, 1]], np.float32)
    total, count, nan, above = pr.reduce_rows(sim, pr.counted(4, 4, self_mode=True), 0.0)
    assert total.tolist() == [0.75, 0.5, 0.0, 0.25] and count.tolist() == [2, 2, 0, 2] and nan.tolist() == [1, 1, 3, 1]
    assert above.tolist() == [2, 2, 0, 2]                                                 # an exact 0 reaches the threshold 0; a NaN never
    assert count.sum() % 2 == 0 and nan.sum() % 2 == 0                                     # the pair relation is symmetric
    valid = [1, 1, 1, 0]
    total, count, nan, _ = pr.reduce_rows(sim, pr.counted(4, 4, valid, valid, self_mode=True), 0.0)
    assert total.tolist() == [0.5, 0.5, 0.0, 0.0] and count.tolist() == [1, 1, 0, 0] and nan.tolist() == [1, 1, 2, 0]
    groups = [-7, 5, -7, 5]                                                                # any int32 is an ordinary id
    total, count, nan, _ = pr.reduce_rows(sim, pr.counted(4, 4, None, None, groups, groups, True), 0.0)
    assert total.tolist() == [0.0, 0.0, 0.0, 0.0] and count.tolist() == [0, 1, 0, 1] and nan.tolist() == [1, 0, 1, 0]
    assert not pr.counted(4, 4, None, None, [0, 1, 2, 3], [0, 1, 2, 3], True).any()        # all distinct: nothing counts
    # two sets: a NULL group side is id 0
    on = pr.counted(2, 4, None, [1, 1, 0, 1], None, [0, 3, 0, 0])
    assert on.tolist() == [[True, False, False, True]] * 2
    # from rows: a row whose harmony part is 0 / 0 gives NaN with everybody, itself included; orthogonal rows give exactly 0
    v = ev.unit_vectors(np.random.default_rng(1), 4)
    v[2, 44:] = np.nan
    v[3, 44:] = 0
    total, count, nan, above = pr.pair_stats(v, threshold=0.0)
    assert count.tolist() == [2, 2, 0, 2] and nan.tolist() == [1, 1, 3, 1] and total[3] == 0 and above.tolist() == [2, 2, 0, 2]
    s01 = ev.sim32(v[:1], v[1:2])[0, 0]
    assert total[0] == float(s01) and total[1] == float(s01)


def gen_batches():
    """the recorded generation trials of the fixture -> (tokens [8, L], mask [8, L]) per trial, as meta_to_batch masks them"""
    f = fixture()
    tokens = f["gen_tokens"].reshape(3, 8, -1)
    mask = np.ones_like(tokens[0])
    mask[:, :len(f["gen_prefix"]) + 1] = 0
    return [(t, mask) for t in tokens]


def test_restatement_of_evaluate_generated_and_totals_on_the_recorded_trials():
    """the reference recorded how many rows of each trial decode; the restatement agrees, and its totals add up"""
    f = fixture()
    totals, seen = pr.GenTotals(), []
    for n, (tokens, mask) in enumerate(gen_batches()):
        m = pr.evaluate_generated(tokens, mask)
        assert m["valid_count"] == f["gen_counts"][n] and m["fatal"] == 0 and not m["vec"][~m["valid"]].any()
        totals.update(m["vec"], m["valid"], m["counts"], groups=np.full(8, n))
        seen.append(m)
    s, tol = totals.summary()
    per_trial = [int(c) * (int(c) - 1) // 2 for c in f["gen_counts"]]                       # grouped by trial: pairs within a trial only
    assert s["valid"] == 14 and s["pairs"] + s["nan_pairs"] == sum(per_trial) and 0 <= s["diversity"] <= 1 and tol["diversity"] < 1e-12
    assert s["cp"] == sum(m["counts"][1] for m in seen) / sum(m["counts"][0] for m in seen)
    one = pr.GenTotals()
    for m in seen:
        one.update(m["vec"], m["valid"], m["counts"])
    assert one.summary()[0]["pairs"] + one.summary()[0]["nan_pairs"] == 14 * 13 // 2


# ------------------------------------------------------------------------------------------------------------------ the bound
def _sequential(terms, dtype=np.float64):
    acc = dtype(0)
    for t in terms:
        acc = dtype(acc + dtype(t))
    return acc


def test_float64_accumulation_in_any_partition_stays_within_gamma_of_fsum():
    """what the kernel does to a row - each lane adds its slice in ascending order, one thread adds the partials in ascending order - for
    every number of slices it can launch with, against the exact sum; the control: an fp32 accumulator breaks the same bound"""
    g = np.random.default_rng(3)
    broke32 = 0
    for n in (1, 2, 3, 17, 128, 129, 1000, 4095):
        s = (g.random(n) * (g.random(n) < 0.7)).astype(np.float32)
        if n > 3:
            s[:3] = [1.0, np.float32(1 - 2.0 ** -16), 1e-13]
        exact = math.fsum(s.astype(np.float64).tolist())
        tol = float(pr.gamma(n)) * float(np.abs(s.astype(np.float64)).sum())
        assert n > 1 or tol == 0
        for parts in (1, 4, 8, 16):
            tile_rows = 128 // parts
            partial = []
            for p in range(parts):                            # part p walks rows [p * tile_rows, (p + 1) * tile_rows) of every tile of 128
                idx = [j for j in range(n) if (j % 128) // tile_rows == p]
                partial.append(_sequential(s[idx]))
            assert abs(float(_sequential(partial)) - exact) <= tol, (n, parts)
        broke32 += abs(float(_sequential(s, np.float32)) - exact) > tol
    assert broke32 >= 3
    assert float(pr.gamma(0)) == float(pr.gamma(1)) == 0 and float(pr.gamma(2)) == pr.U / (1 - pr.U)


# ------------------------------------------------------------------------------------------------------------------ the threshold
def _self_similarity(v):
    out = []
    for lo in range(0, len(v), 100):
        out.append(np.diagonal(ev.sim32(v[lo:lo + 100], v[lo:lo + 100])))
    return np.concatenate(out).astype(np.float64)


def test_identical_pieces_reach_the_default_duplicate_threshold():
    """1 - 2^-16 is derived: (3 n + 6) 2^-24 per part gives 188 * 2^-24 < 2^-16.  Measured on the fp32 operation order: the
    self-similarity of 3000 unit-norm rows and of every finite row of the fixture is at most 6 * 2^-24 below 1"""
    assert evaluation.GenerationTotals.__init__.__defaults__[1] == pr.DEFAULT_THRESHOLD == 1 - 2.0 ** -16
    assert float(np.float32(pr.DEFAULT_THRESHOLD)) == pr.DEFAULT_THRESHOLD                 # exact in fp32: the kernel compares in fp32
    assert sum(3 * n + 6 for n in (32, 12, 12)) + 2 == 188 and 188 * 2.0 ** -24 < 2.0 ** -16
    s = _self_similarity(ev.unit_vectors(np.random.default_rng(21), 3000))
    assert (1 - s <= 6 * 2.0 ** -24).all() and (s >= pr.DEFAULT_THRESHOLD).all(), float((1 - s).max()) * 2 ** 24
    vec = fixture()["vec"]
    vec = vec[~np.isnan(vec).any(1)]
    assert len(vec) == 75
    s = _self_similarity(vec)
    assert (1 - s <= 6 * 2.0 ** -24).all() and (s >= pr.DEFAULT_THRESHOLD).all(), float((1 - s).max()) * 2 ** 24


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    L = _lib.lib()
    buf = (C.c_float * 112)()
    ints = (C.c_int32 * 8)()
    dbl = (C.c_double * 2)()
    a, m, s = C.addressof(buf), C.addressof(ints), C.addressof(dbl)
    ok = dict(q=a, nq=2, k=a, nk=2, qv=None, kv=None, qg=None, kg=None, self=0, thr=0.5, sum=s, count=m, nan=m + 8, above=m + 16)
    bad = [dict(q=None), dict(k=None), dict(sum=None), dict(count=None), dict(nan=None), dict(nq=0), dict(nk=0), dict(nq=-1), dict(nk=1 << 26),
           dict(nq=1 << 26), dict(self=2), dict(self=-1), dict(self=1, k=a + 224, nk=1, nq=1), dict(self=1, nk=1), dict(self=1, qv=m),
           dict(self=1, kv=m), dict(self=1, qg=m), dict(self=1, kg=m), dict(self=1, qg=m, kg=m + 8)]
    for change in bad:
        args = {**ok, **change}
        assert L.mhs_msim_pair_stats(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"msim_pair_stats" in L.mh_last_error()
        if change.get("self") == 1:
            assert b"self = 1" in L.mh_last_error()


# ------------------------------------------------------------------------------------------------------------------ the driver
TABLE = ev.unit_vectors(np.random.default_rng(8), 6)


class StubDecodedRows(StubDecoded):
    """+ what evaluate_generated reads of a DecodedBatch"""

    def __init__(self, status, tokens):
        super().__init__(status)
        self.restored, self.lengths, self.meta = tokens, None, None


@pytest.fixture
def stub(monkeypatch):
    """decode: the row's status is its first token; its vector is row (second token) of TABLE; CP (valid, 1), CV (10 valid, valid); the
    kernels behind metric.pair_stats / metric.nearest are the numpy restatement"""
    calls = {"decode": [], "pair_stats": 0, "nearest": 0}

    def decode_tokens(tokens, mask, strict_validation=False, **kw):
        calls["decode"].append(bool(strict_validation))
        return StubDecodedRows(tokens[:, 0].to(torch.int32), tokens)

    def counts(meta, tokens, lengths=None, valid=None):
        n = valid.sum()
        return torch.stack([n, torch.ones_like(n), 10 * n, n])

    def pair_stats(vec, keys=None, valid=None, keys_valid=None, groups=None, keys_groups=None, threshold=None):
        calls["pair_stats"] += 1
        assert keys is None
        out = pr.pair_stats(vec.numpy(), None, valid.numpy(), None, groups.numpy(), None, threshold)
        return metric.PairStats(*[None if x is None else torch.from_numpy(x) for x in out])

    def nearest(vec, keys=None, valid=None, keys_valid=None, return_values=False, return_sim=False):
        calls["nearest"] += 1
        most, best, _ = ev.nearest(vec.numpy(), keys.numpy(), valid.numpy(), None if keys_valid is None else keys_valid.numpy())
        return [torch.from_numpy(most), torch.from_numpy(best)]

    monkeypatch.setattr(du, "decode_tokens", decode_tokens)
    monkeypatch.setattr(metric, "get_vectors", lambda tokens, lengths=None, **kw: torch.from_numpy(TABLE[tokens[:, 1].numpy()]))
    monkeypatch.setattr(metric, "controllability_counts", counts)
    monkeypatch.setattr(metric, "pair_stats", pair_stats)
    monkeypatch.setattr(metric, "nearest", nearest)
    monkeypatch.setattr(du, "meta_to_batch", lambda meta, B, L, device="cuda": {"input_ids": torch.zeros(B, L, dtype=torch.int32),
                                                                             "input_mask": torch.ones(B, L, dtype=torch.int32)})
    return calls


TRIALS = [([du.NO_EOS] * 4, [0, 1, 2, 3]), ([du.OK, du.NO_EOS, du.OK, du.ONCE_FAILED], [0, 0, 1, 1]), ([du.OK] * 4, [2, 0, 3, 4]),
          ([du.OK] * 4, [5, 5, 5, 5])]


def _sampler():
    trials = iter(TRIALS)

    def sample(cond):
        st, which = next(trials)
        t = _rows(st)
        t[:, 1] = torch.tensor(which)
        return t
    return sample, trials


def test_run_generation_with_metrics_numbers_files_as_without(stub, tmp_path):
    logs, reps = {}, {}
    for on in (False, True):
        sample, trials = _sampler()
        logs[on] = []
        reps[on] = sampling.run_generation(None, None, META, batch_size=4, seq_len=6, num_samples=5, out_dir=str(tmp_path / str(on)),
                                           log=logs[on].append, sampler=sample, device="cpu", get_metric=on, corpus=torch.from_numpy(TABLE[4:]) if on else None)
        assert next(trials)[1] == [5, 5, 5, 5]                 # 0 + 2 + 4 = 6 >= 5: both stop after the third batch
        logs[on] = [ln.replace(str(tmp_path / str(on)), "<out>") for ln in logs[on]]
    off, rep = reps[False], reps[True]
    assert (rep.total_valid_count, rep.batches) == (off.total_valid_count, off.batches) == (6, 3)
    assert sorted(os.listdir(tmp_path / "True")) == sorted(os.listdir(tmp_path / "False")) == ["generated_%07d.midi" % n for n in range(6)]
    assert off.totals is None and off.summary is None and stub["decode"] == [False] * 6
    assert stub["pair_stats"] == 1 and stub["nearest"] == 1, "one call each, at the end of the run"
    # the log: the same lines, plus the announcement and the summary block
    extra = [ln for ln in logs[True] if ln not in logs[False]]
    assert [ln for ln in logs[True] if ln in logs[False]] == logs[False] and len(extra) == 2
    assert extra[0] == "### with calculating metrics ..." and extra[1] == evaluation.generation_block(rep.summary)
    assert logs[True].index(extra[1]) == len(logs[True]) - 2 and " Summary: Generation " in extra[1]
    # the summary is the restatement's: valid rows 0, 2 of the second batch and all of the third - vectors 0, 1 | 2, 0, 3, 4
    want = pr.GenTotals(corpus=TABLE[4:])
    for st, which in TRIALS[:3]:
        valid = np.array(st) == du.OK
        want.update(TABLE[which], valid, (valid.sum(), 1, 10 * valid.sum(), valid.sum()))
    want, _ = want.summary()
    assert set(rep.summary) == {"valid", "pairs", "nan_pairs", "diversity", "duplicates", "cp", "cv", "novelty", "memorised"}
    assert rep.summary == pytest.approx(want, rel=1e-12) and rep.totals.summary() == rep.summary
    assert rep.summary["valid"] == 6 and rep.summary["pairs"] == 15 and rep.summary["nan_pairs"] == 0
    assert rep.summary["duplicates"] == 2 / 6 and rep.summary["memorised"] == 1 / 6        # vector 0 twice; vector 4 is in the corpus
    assert 0 < rep.summary["diversity"] < 1 and rep.summary["cp"] == 3 / 6 and rep.summary["cv"] == 6 / 60
    assert "Duplicates: 0.333333" in extra[1] and "Memorised: 0.166667" in extra[1] and "Valid: 6" in extra[1]


def test_run_generation_with_metrics_and_no_valid_row(stub, tmp_path):
    log = []
    rep = sampling.run_generation(None, None, META, batch_size=4, seq_len=6, num_samples=5, out_dir=None, max_batches=2, log=log.append,
                                  sampler=lambda cond: _rows([du.NO_EOS] * 4), device="cpu", get_metric=True, duplicate_threshold=0.5)
    assert rep.total_valid_count == 0 and rep.batches == 2 and rep.totals.duplicate_threshold == 0.5
    s = rep.summary
    assert s["valid"] == 0 and s["pairs"] == 0 and all(math.isnan(s[k]) for k in ("diversity", "duplicates", "cp", "cv")) and "novelty" not in s
    # a fatal status raises at the summary what MetricTotals raises
    totals = evaluation.GenerationTotals("cpu")
    totals.fatal = torch.tensor(du.REF_INDEXERROR, dtype=torch.int32)
    with pytest.raises(IndexError):
        totals.summary()
