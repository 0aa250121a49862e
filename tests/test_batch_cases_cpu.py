"""CPU: the edge-case list of the batch / validator / metric kernels (tests/batch_cases.py) is what it claims to be, and the numpy oracle
(oracle/batch.py) agrees with the REFERENCE on every short edge row - outputs bit for bit (MSIM vectors: the tolerance
tests/test_batch_cpu.py uses) and exceptions: the oracle raises if and only if the reference raised (tests/golden/batch_edges.npz,
written by tools/make_golden_batch_edges.py).  That is what lets tests/test_batch_matrix_gpu.py use the oracle on the long rows."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import batch_cases as bc
from conftest import REPO, load_golden
from oracle import batch as ob


@pytest.fixture(scope="module")
def g():
    return load_golden("batch_edges.npz")


def seg(g, key, off, i):
    return g[key][g[off][i]:g[off][i + 1]]


def attempt(fn):
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return fn(), False
    except (AssertionError, IndexError, UnboundLocalError):
        return None, True


# ------------------------------------------------------------------------------------------------ oracle == reference on the fixture
@pytest.mark.parametrize("fam", ["mt", "mn", "rn", "rr"])
def test_corruption_oracle_matches_reference_on_edge_rows(g, fam):
    rows = bc.stored_rows(fam)
    assert len(rows) == len(g[fam + "_names"]) > 0
    for i, (b, r) in enumerate(rows):
        name = "%s/%s" % (b["name"], r["name"])
        assert g[fam + "_names"][i] == name
        assert np.array_equal(seg(g, fam + "_values", fam + "_offsets", i), r["seq"]), name          # the fixture is of this case list
        raised = bool(g[fam + "_exc"][i])
        if fam == "rr":
            assert np.array_equal(seg(g, "rr_pairs", "rr_pairs_offsets", i), r["pairs"]) and g["rr_count"][i] == b["count"], name
        else:
            k = int(g[fam + "_draws"][i])                                                            # the draws the reference consumed
            assert np.array_equal(seg(g, fam + "_u", fam + "_offsets", i)[:k], r["u"][:k]), name
            if fam != "mt":
                assert k == len(ob._eligible_velocity(r["seq"])), name                               # rank, not position, counts draws
            assert not raised, name
        got, threw = attempt(lambda: bc.oracle_row(fam, b, r))
        assert threw == raised, (name, threw, int(g[fam + "_exc"][i]))
        if not raised:
            assert np.array_equal(got, seg(g, fam + "_out", fam + "_out_offsets", i)), name
            if fam == "rn":                                                                          # and with the draws as the Recorder logged them
                u, new = seg(g, "rn_u", "rn_offsets", i), seg(g, "rn_new", "rn_offsets", i)
                assert np.array_equal(ob.randomize_note(r["seq"], u, new, np.float32(b["p"])), got), name


def test_masking_note_clears_the_last_token_of_a_three_token_row(g):
    """the reference's corrupted[idx-1 : idx+3] at idx = 0 is seq[-1:3]: empty, except in a row of exactly 3 tokens, where it is seq[2:3]"""
    i = list(g["mn_names"]).index("edges/n3_vel0_fires")
    a, out = seg(g, "mn_values", "mn_offsets", i), seg(g, "mn_out", "mn_out_offsets", i)
    assert len(a) == 3 and 131 <= a[0] <= 194 and out.tolist() == [a[0], a[1], 0]
    j = list(g["mn_names"]).index("edges/n4_vel0_fires")
    assert np.array_equal(seg(g, "mn_values", "mn_offsets", j), seg(g, "mn_out", "mn_out_offsets", j))


def test_flagged_rotations_are_where_the_reference_raises_or_changes_the_row_length(g):
    """the pinned divergence of random_rotating: where the kernel sets status 1 on a pair the reference could draw, the reference either
    raises (no EOS: IndexError; fewer than two bars: AssertionError) or returns a row of another length (last EOS before the second bar).
    With count = 0 the reference's loop and its assert never run: it returns the row, and so does the kernel, flagged all the same"""
    seen = set()
    for i, (b, r) in enumerate(bc.stored_rows("rr")):
        n_out = int(g["rr_out_offsets"][i + 1] - g["rr_out_offsets"][i])
        if r["status"] == 0:
            assert g["rr_exc"][i] == 0 and n_out == len(r["seq"]), r["name"]
        elif b["count"] == 0:
            assert r["name"] == "c0_one_bar" and g["rr_exc"][i] == 0 and np.array_equal(seg(g, "rr_out", "rr_out_offsets", i), r["seq"])
        else:
            assert g["rr_exc"][i] != 0 or n_out != len(r["seq"]), r["name"]
            seen.add((r["name"], int(g["rr_exc"][i])))
    assert seen == {("one_bar", bc.EXC["AssertionError"]), ("no_bar", bc.EXC["AssertionError"]), ("no_eos", bc.EXC["IndexError"]),
                    ("eos_before_second_bar", 0)}


def test_collate_and_meta_to_batch_match_reference_on_edge_rows(g):
    rows = bc.stored_rows("r2p")
    assert len(rows) == len(g["r2p_names"]) > 0
    seen_raise = False
    for i, (b, r) in enumerate(rows):
        exp, length = bc.r2p_expected(dict(b, rows=[r]))
        if g["r2p_exc"][i]:                                # the reference raises on a row longer than seq_len; the kernel truncates (pinned)
            assert len(r["seq"]) > b["L"]
            seen_raise = True
        else:
            assert len(r["seq"]) <= b["L"]
            assert np.array_equal(seg(g, "r2p_out", "r2p_out_offsets", i), exp[0]) and g["r2p_length"][i] == length[0]
            col = ob.collate([r["seq"]], [r["seq"]], [r["seq"]], b["L"])
            assert np.array_equal(col["input_mask" if b["pad"] else "input_ids"][0], exp[0])
    assert seen_raise
    rows = bc.stored_rows("m2b")
    assert len(rows) == len(g["m2b_names"]) > 0
    for i, (b, _) in enumerate(rows):
        ids, msk = ob.meta_to_batch(b["meta"], b["B"], b["L"])
        assert np.array_equal(seg(g, "m2b_meta", "m2b_meta_offsets", i), b["meta"])
        assert np.array_equal(seg(g, "m2b_ids", "m2b_out_offsets", i), ids.ravel()) and np.array_equal(seg(g, "m2b_mask", "m2b_out_offsets", i), msk.ravel())


def test_validator_oracle_matches_reference_on_edge_rows(g):
    rows = bc.stored_rows("val")
    assert len(rows) == len(g["val_names"]) > 0
    classes = set()
    for i, (b, r) in enumerate(rows):
        assert np.array_equal(seg(g, "val_tokens", "val_offsets", i), r["seq"]) and g["val_len"][i] == r["len"]
        got = ob.validate(r["seq"], r["len"])
        assert got == tuple(int(v) for v in g["val_result"][i]), (r["name"], got, g["val_result"][i])
        classes.add("no eos" if got[0] < 0 else got[1:])
    assert classes >= {(0, 1), (0, 0), (1, 0), (0, -2), (1, 1), (1, -2), "no eos"}
    eos = {r["name"]: int(g["val_result"][i][0]) for i, (b, r) in enumerate(rows)}
    assert [eos[k] for k in ("eos0", "eos63", "eos64", "eos65", "eos_last", "len0", "eos_beyond_len")] == [0, 63, 64, 65, 79, -1, -1]


def test_msim_oracle_matches_reference_on_edge_rows(g):
    rows = bc.stored_rows("msim")
    assert len(rows) == len(g["msim_names"]) > 0
    codes = {}
    for i, (b, r) in enumerate(rows):
        assert np.array_equal(seg(g, "msim_tokens", "msim_offsets", i), r["seq"]) and g["msim_len"][i] == r["len"]
        raised = bool(g["msim_exc"][i])
        got, threw = attempt(lambda: ob.msim_vectors(r["seq"][:r["len"]], b["note_len"]))
        assert threw == raised, (r["name"], threw, int(g["msim_exc"][i]))
        codes[r["name"]] = int(g["msim_exc"][i])
        assert bc.msim_status(r) == r["status"], r["name"]
        if codes[r["name"]] == bc.EXC["UnboundLocalError"]:    # no position token between the first BAR and the EOS: the pinned divergence below
            assert r["status"] == 0 and r["name"] in ("bar_then_eos", "bars_only"), r["name"]
            continue
        assert raised == (r["status"] != 0), r["name"]     # the kernel flags exactly the rows the reference raises on
        if not raised:
            ref = g["msim_vectors"][i]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), r["name"]
            ok = ~np.isnan(ref)
            np.testing.assert_allclose(got[ok], ref[ok], rtol=2e-6, atol=2e-7, err_msg=r["name"])
    E = bc.EXC
    assert codes["bar_then_eos"] == codes["bars_only"] == E["UnboundLocalError"] and codes["no_bar"] == E["IndexError"]
    assert codes["position_then_garbage"] == E["ValueError"] and codes["off_end_mid_note"] == E["IndexError"] and codes["off_end_no_eos"] == E["IndexError"]
    # BAR then EOS: the reference raises UnboundLocalError, the kernel is pinned to status 0 with flat rhythm / melody and NaN harmony
    row = next(r for _, r in rows if r["name"] == "bar_then_eos")
    v = bc.msim_expected(row, 128.0)
    assert bc.msim_status(row) == 0 and np.allclose(v[:32], 32 ** -0.5) and np.allclose(v[32:44], 12 ** -0.5) and np.isnan(v[44:]).all()
    chord = next(r for _, r in rows if r["name"] == "chord_only")
    i = list(g["msim_names"]).index("B65/chord_only")
    assert np.isnan(g["msim_vectors"][i][44:]).all() and not np.isnan(g["msim_vectors"][i][:44]).any() and chord["status"] == 0


def test_controllability_oracle_matches_reference_on_edge_rows(g):
    rows = bc.stored_rows("ctrl")
    assert len(rows) == len(g["ctrl_names"]) > 0
    for i, (b, r) in enumerate(rows):
        assert np.array_equal(seg(g, "ctrl_tokens", "ctrl_offsets", i), r["seq"]) and np.array_equal(g["ctrl_metas"][i], r["meta"][:11])
        assert g["ctrl_exc"][i] == 0, r["name"]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            (pt, pw), (vt, vw) = ob.controllability([r["meta"]], [r["seq"][:r["len"]]])
        assert [pt, pw] == g["ctrl_pitch"][i].tolist() and [vt, vw] == g["ctrl_velocity"][i].tolist(), r["name"]
        # the per-row counters the kernel returns give the same verdicts
        psum, pcnt, vtot, vbad = (int(v) for v in bc.ctrl_counts(r))
        if int(r["meta"][8]) - 524 != 130:
            assert [vtot, vbad] == [vt, vw], r["name"]
        if int(r["meta"][3]) != 630:
            lo, hi = ob.PITCH_RANGE[int(r["meta"][3])]
            assert (not (pcnt and lo <= psum / pcnt <= hi)) == bool(pw), r["name"]
    no_pitch = list(g["ctrl_names"]).index("L80/no_pitch")
    assert g["ctrl_pitch"][no_pitch].tolist() == [1, 1]              # the reference's NaN mean counts as wrong


# ------------------------------------------------------------------------------------------------------ conditions on the case list
def test_every_entry_point_of_batch_hip_has_cases():
    src = open(os.path.join(REPO, "musediffusion_amd", "csrc", "batch.hip")).read()
    entries = set(re.findall(r'extern "C" \w+ (mh_\w+)\(', src))
    assert entries - {"mh_batch_max_row"} == set(bc.ENTRY.values()) and "mh_batch_max_row" in entries
    fams = bc.families()
    assert set(fams) == set(bc.ENTRY)
    for fam, batches in fams.items():
        assert batches and all(b["rows"] for b in batches), fam
        assert all(len(b["rows"]) <= 65 for b in batches), fam
        names = [(b["name"], r["name"]) for b in batches for r in b["rows"]]
        assert len(set(names)) == len(names), fam
    assert int(re.search(r"constexpr int MAX_ROW = (\d+);", src).group(1)) == bc.MAX_ROW
    assert int(re.search(r"constexpr int TB = (\d+);", src).group(1)) == bc.TB
    assert any(len(b["rows"]) == 1 for b in fams["mt"]) and all(any(len(b["rows"]) == 1 for b in fams[f]) for f in ("mn", "rr", "val", "msim", "ctrl", "r2p"))


def test_row_lengths_stay_within_the_limit_except_the_one_oversize_row():
    over = [(fam, r["name"]) for fam in ("mt", "mn", "rn", "rr", "r2p", "val", "msim", "ctrl") for b in bc.families()[fam] for r in b["rows"]
            if len(r["seq"]) > bc.MAX_ROW]
    assert over == [("rr", "len4097")]
    assert max(len(r["seq"]) for b in bc.families()["rr"] for r in b["rows"]) == bc.MAX_ROW + 1


def test_masking_token_cases_sit_on_the_seams():
    rows = {r["name"]: (b, r) for b in bc.families()["mt"] for r in b["rows"]}
    assert sorted({len(r["seq"]) for _, r in rows.values()} & {0, 5, 12, 13, 268, 4096}) == [0, 5, 12, 13, 268, 4096]
    first = lambda r: next((j for j in range(12, len(r["seq"])) if r["seq"][j] == 1), None)
    assert [first(rows[k][1]) for k in ("eos12", "eos267", "eos268", "eos269", "eos_last_268", "len4096_eos_last")] == [12, 267, 268, 269, 267, 4095]
    assert first(rows["eos_before12_only"][1]) is None and (rows["eos_before12_only"][1]["seq"][:12] == 1).any()
    assert first(rows["no_eos"][1]) is None and (rows["two_eos"][1]["seq"] == 1).sum() == 2
    u = rows["draw_on_p"][1]["u"]
    assert (u == np.float32(0.3)).any() and (u < np.float32(0.3)).any()
    out = bc.oracle_row("mt", *rows["draw_on_p"])
    keep = np.nonzero(u[:47] == np.float32(0.3))[0] + 12
    assert np.array_equal(out[keep], rows["draw_on_p"][1]["seq"][keep]) and (out[12:59] == 0).sum() == (u[:47] < np.float32(0.3)).sum() > 0
    assert {b["p"] for b in bc.families()["mt"]} >= {0.0, 0.3, 1.0}
    for name in ("p0_a", "p0_b"):                          # p = 0 masks nothing although draws of exactly 0 are there; p = 1 masks the region
        assert (rows[name][1]["u"] == 0).any() and np.array_equal(bc.oracle_row("mt", *rows[name]), rows[name][1]["seq"])
    assert (bc.oracle_row("mt", *rows["p1_a"])[12:49] == 0).all()


def test_note_cases_fire_where_they_say_and_by_rank():
    rows = {r["name"]: (b, r) for b in bc.families()["mn"] for r in b["rows"]}
    assert bc.families()["mn"] is bc.families()["rn"]
    positions = set()
    for name, (b, r) in rows.items():
        seq, elig = r["seq"], ob._eligible_velocity(r["seq"])
        fired = [idx for k, idx in enumerate(elig) if r["u"][k] < np.float32(b["p"])]
        positions |= set(fired)
        positions |= {idx - len(seq) for idx in fired}                  # negative: distance from the end
        # by position instead of rank the same draws would fire another set (wherever rank != position for some token)
        by_pos = [idx for idx in elig if r["u"][idx] < np.float32(b["p"])]
        if fired and any(k != idx for k, idx in enumerate(elig)) and not name.startswith(("all_vel", "p1_", "tail_mixed", "overlap", "n3_", "sparse")):
            assert by_pos != fired, name
        for v in r["vel"]:
            assert 131 <= seq[v] <= 194
    assert positions >= {0, 1, 254, 255, 256, 257, 511, 512, 513, -3}
    b, r = rows["tail_not_eligible"]
    assert ob._eligible_velocity(r["seq"]) == [] and (r["u"] < 0.5).all()
    assert np.array_equal(bc.oracle_row("mn", b, r), r["seq"]) and np.array_equal(bc.oracle_row("rn", b, r), r["seq"])
    b, r = rows["seam_all"]                                             # overlapping windows: the largest firing index at or below j wins
    out = bc.oracle_row("rn", b, r)
    k257 = ob._eligible_velocity(r["seq"]).index(257)
    assert out[257:260].tolist() == r["new"][k257].tolist() and out[256] == r["new"][k257 - 1][0] and out[255] == r["new"][k257 - 2][0]
    for n in (256, 257, 4096):
        assert ((rows["all_vel_%d" % n][1]["seq"] >= 131) & (rows["all_vel_%d" % n][1]["seq"] <= 194)).all() and len(rows["all_vel_%d" % n][1]["seq"]) == n
    batch = bc.families()["mn"][0]["rows"]
    i = [r["name"] for r in batch].index("empty_between")
    assert len(batch[i]["seq"]) == 0 and len(batch[i - 1]["seq"]) > 12 and len(batch[i + 1]["seq"]) > 12


def test_rotation_cases_and_the_flagged_list():
    rows = [(b, r) for b in bc.families()["rr"] for r in b["rows"]]
    flagged = [r["name"] for b, r in rows if r["status"] != 0]
    assert sorted(flagged) == sorted(bc.RR_FLAGGED)                     # exactly the explicit list: nothing else ends up flagged
    assert {b["count"] for b, _ in rows} == {0, 1, 3}
    for b, r in rows:
        assert r["pairs"].shape == (b["count"], 2) and r["status"] == bc.rr_status(r["seq"], r["pairs"])
        if r["status"] == 0:                                            # the oracle rotates every compare-class row, keeping its length
            out = bc.oracle_row("rr", b, r)
            assert len(out) == len(r["seq"]) and np.array_equal(np.sort(out), np.sort(r["seq"])), r["name"]
    by = {r["name"]: r for _, r in rows}
    bars = lambda r: np.nonzero(r["seq"] == 2)[0]
    assert 255 in bars(by["bar_at_255"]) and 256 in bars(by["bar_at_256"])
    s = bars(by["bar_straddles_256"])
    assert any(a < 255 and 256 < b_ for a, b_ in zip(s[:-1], s[1:]) if (b_ - a) < 20)
    assert len(bars(by["two_bars"])) == 2 and by["last_bar_second"]["pairs"][:, 1].max() == len(bars(by["last_bar_second"])) - 1
    assert (np.diff(by["adjacent"]["pairs"], axis=1) == 1).all() and len({tuple(p) for p in by["same_pair"]["pairs"]}) == 1
    for name in ("many_bars_a", "many_bars_b"):
        r = by[name]
        assert len(r["seq"]) == bc.MAX_ROW and len(bars(r)) == 2100 and r["pairs"].min() < 2048 <= r["pairs"].max() and r["status"] == 0
        assert not np.array_equal(bc.oracle_row("rr", {"count": 3}, r), r["seq"])
    assert by["len4097"]["status"] == 2
    for name in bc.RR_FLAGGED:                                          # flagged and oversize rows have compare-class neighbours
        order = next([r["name"] for r in b["rows"]] for b in bc.families()["rr"] if any(r["name"] == name for r in b["rows"]))
        i = order.index(name)
        assert by[order[i - 1]]["status"] == 0 or by[order[i + 1]]["status"] == 0, name
        if name == "len4097":
            assert by[order[i + 1]]["status"] == 0


def test_padded_and_meta_cases():
    b = bc.families()["r2p"]
    assert {x["L"] for x in b} >= {1, 255, 256, 257} and {x["pad"] for x in b} == {0, 1} and any(not x["with_length"] for x in b)
    for x in b[:-1]:
        lens = [len(r["seq"]) for r in x["rows"]]
        assert 0 in lens and x["L"] in lens and max(lens) > x["L"]
        out, length = bc.r2p_expected(x)
        i = lens.index(max(lens))
        assert length[i] == max(lens) and np.array_equal(out[i], x["rows"][i]["seq"][:x["L"]])      # truncated, length reports n
    m = bc.families()["m2b"]
    assert {(x["L"], len(x["meta"])) for x in m} >= {(40, 0), (40, 39), (40, 40)}
    assert any(x["B"] * x["L"] == 4096 * 256 + 257 for x in m)


def test_counter_and_validator_cases_sit_on_the_wave_seams():
    rows = [r for b in bc.families()["ctrl"] for r in b["rows"]]
    seen = {(int(r["seq"][j]), j) for r in rows if r["name"].startswith("tok") for j in (63, 64, 65) if r["seq"][j] != 300}
    assert seen == {(t, j) for t in (2, 3, 130, 131, 194, 195) for j in (63, 64, 65)}
    by = {r["name"]: r for r in rows}
    assert bc.ctrl_counts(by["no_pitch"])[1] == 0 and bc.ctrl_counts(by["no_pitch"])[2] > 0 and by["len0"]["len"] == 0
    assert by["lo_open"]["meta"][7] - 524 == 130 and by["hi_open"]["meta"][8] - 524 == 195
    assert bc.ctrl_counts(by["bounds_inclusive"]).tolist()[2:] == [4, 2]
    assert any(b["meta_ld"] > 11 for b in bc.families()["ctrl"]) and any(not b["use_lens"] for b in bc.families()["ctrl"])
    assert bc.ctrl_counts(by["len4096_all_pitch"]).tolist() == [130 * 4096, 4096, 0, 0]
    ms = bc.families()["msim"]
    assert {len(b["rows"]) for b in ms} >= {1, 64, 65} and {b["note_len"] for b in ms} > {128.0} and any(not b["use_lens"] for b in ms)
    st = {r["name"]: r["status"] for b in ms for r in b["rows"]}
    assert st["no_bar"] == 1 and st["position_then_garbage"] == st["off_end_mid_note"] == st["off_end_no_eos"] == 2 and st["chord_only"] == 0
    assert any(not b["use_lens"] for b in bc.families()["val"])


# ----------------------------------------------------------------------------------------------------------- _draw_bar_pairs (pure torch)
def test_draw_bar_pairs_are_sorted_distinct_in_range_and_uniform():
    from musediffusion_amd.data.corruption import _draw_bar_pairs
    mk = lambda nbar: [2, 440, 200] * nbar + [1]
    rows = [mk(4), mk(1), mk(0), mk(2), mk(7), [], mk(3)]
    nbar = torch.tensor([4, 1, 0, 2, 7, 0, 3])
    values = torch.tensor([t for r in rows for t in r], dtype=torch.int32)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), dtype=torch.int64)
    torch.manual_seed(11)
    pairs = _draw_bar_pairs(values, offsets, 500)
    assert pairs.shape == (7, 500, 2) and pairs.dtype == torch.int32
    lim = nbar.clamp(min=2).view(-1, 1)
    assert bool((pairs[..., 0] >= 0).all() and (pairs[..., 0] < pairs[..., 1]).all() and (pairs[..., 1] < lim).all())
    for b in (1, 2, 3, 5):                                 # fewer than two bars (and exactly two): (0, 1), which the kernel then flags or swaps
        assert bool((pairs[b] == torch.tensor([0, 1], dtype=torch.int32)).all())
    assert len({tuple(p) for p in pairs[4].tolist()}) == 21 and len({tuple(p) for p in pairs[6].tolist()}) == 3
    # a row of 4 bars: the 6 pairs are equally likely - each count within 6 binomial standard deviations of N / 6
    N = 60000
    v4, o4 = torch.tensor(mk(4), dtype=torch.int32), torch.tensor([0, len(mk(4))], dtype=torch.int64)
    torch.manual_seed(12)
    p = _draw_bar_pairs(v4, o4, N)[0].long()
    counts = torch.bincount(p[:, 0] * 4 + p[:, 1], minlength=16)
    want = [0 * 4 + 1, 0 * 4 + 2, 0 * 4 + 3, 1 * 4 + 2, 1 * 4 + 3, 2 * 4 + 3]
    assert int(counts[want].sum()) == N
    sd = (N * (1 / 6) * (5 / 6)) ** 0.5
    assert all(abs(int(counts[k]) - N / 6) <= 6 * sd for k in want), counts[want].tolist()
