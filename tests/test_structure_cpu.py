"""CPU: the structure rule without a device.  tests/structure_ref.py (the plain-Python restatement of csrc/structure.hip) on hand-made
rows with answers worked out here, on the slot and bar seams of all four time signatures, on the notes the rule skips and on every
status; the table route to an entropy against the direct formula under a derived bound; the reference's own recorded notes of
tests/golden/decode.npz; evaluation.StructureTotals.ratios and structure_gap on host vectors; the refusals of the entry point, which
come before any launch.  No kernel runs here: the device side is tests/test_structure_gpu.py and tests/test_structure_sampling_gpu.py.

The bound of the table route.  H = (T[N] - S) / N with T[k] = fl(k fl(log2 k)).  Each table entry carries two roundings and log2's own
error (below one ulp), S eleven more additions of non-negative terms, then one subtraction and one division: fewer than 32 roundings
of quantities that are at most T[N] + S, hence |H - H_exact| <= 32 * 2^-53 * (T[N] + S) / N, plus 2^-52 for the direct formula's own
rounding (math.fsum of twelve correctly rounded products below 0.54 each)."""
import ctypes as C
import math

import numpy as np
import pytest

import decode_ref as dr
import structure_ref as sr
from musediffusion_amd import _lib, evaluation, metric
from test_decode_cpu import fixture_cases

META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]   # c major, 4/4: 1920 ticks a bar, 16 slots
TABLE = metric.xlog2x_host(32768)
NAMES = metric.STRUCTURE_COUNT_NAMES
LOG2_12 = math.log2(12)


def note(start, pitch, length=100, velocity=64):
    return (start, start + length, pitch, velocity)


def meta_of(ts):
    return META[:2] + [ts] + META[3:]


def counts_of(notes, meta=META, **kw):
    return sr.row_counts(notes, meta, TABLE, **kw)


def named(counts):
    return dict(zip(NAMES, counts))


def ratios_of(*rows):
    """evaluation.StructureTotals.ratios over rows of (counts, entropy), summed on the host"""
    t = sr.Totals()
    for counts, ent in rows:
        t.update(counts, ent)
    return evaluation.StructureTotals.ratios(t.vector())


def bound(hist):
    N = sum(hist)
    S = sum(float(TABLE[c]) for c in hist)
    return 32 * 2.0 ** -53 * (float(TABLE[N]) + S) / N + 2.0 ** -52


def direct(hist):
    N = sum(hist)
    return math.fsum(-(c / N) * math.log2(c / N) for c in hist if c)


def test_names_and_status_codes_mirror_the_header():
    assert (sr.OK, sr.MASKED, sr.BAD_META, sr.BAD_COUNTS) == tuple(range(4))
    assert _lib.ABI["musehip_structure.h"].enums == {"MHM_OK": 0, "MHM_MASKED": 1, "MHM_BAD_META": 2, "MHM_BAD_COUNTS": 3}
    assert (metric.STRUCTURE_OK, metric.STRUCTURE_MASKED, metric.STRUCTURE_BAD_META, metric.STRUCTURE_BAD_COUNTS) == tuple(range(4))
    assert len(NAMES) == 16 and len(set(NAMES)) == 16 and len(metric.STRUCTURE_BAR_NAMES) == 16
    assert (metric.STRUCTURE_MAX_NOTES, metric.STRUCTURE_MAX_BARS) == (32768, 512)
    assert sr.TICKS_PER_BAR == {627 + i: 480 * dr.BEATS[i] for i in range(4)}


def test_the_table():
    t = metric.xlog2x_host(9)
    assert t.dtype == np.float64 and t.shape == (10,) and t[0] == 0.0 and t[1] == 0.0
    assert [float(t[k]) for k in (2, 4, 8)] == [2.0, 8.0, 24.0]                    # exact at the powers of two
    assert all(abs(float(t[k]) - k * math.log2(k)) <= 2.0 ** -52 * k * math.log2(k) for k in range(2, 10))
    assert np.array_equal(TABLE[:10], t) and (np.diff(TABLE[1:]) > 0).all()
    import torch
    dev = metric.xlog2x_table(9, "cpu")
    assert dev.dtype == torch.float64 and np.array_equal(dev.numpy(), t) and metric.xlog2x_table(9, "cpu") is dev, "cached per device and size"


# ------------------------------------------------------------------------------------------------------------------ hand-made rows
def test_one_bar_holding_one_pitch():
    counts, ent, bars, st = counts_of([note(0, 60), note(480, 60), note(960, 72)], max_bars=2)
    c = named(counts)
    assert st == sr.OK and float(ent[0]) == 0.0 and not np.signbit(ent[0]) and float(ent[1]) == 0.0
    assert counts == [3, 0, 1, 1, 1, 2, 60, 72, 3, 0, 0, 16, 1, 0, 0, 0]
    assert bars == [[3, 0b100010001, 60, 72] + [3] + [0] * 11, [0, 0, -1, -1] + [0] * 12]
    assert c["windows_4"] == 0 and sr.gs(counts) is None
    r = ratios_of((counts, ent))
    assert r["h1"] == 0.0 and math.isnan(r["h4"]) and math.isnan(r["gs"]) and r["notes_per_bar"] == 3.0 and r["empty_bars"] == 0.0
    assert (r["pitch_classes"], r["distinct_pitches"], r["pitch_range"], r["onsets_per_bar"]) == (1.0, 2.0, 12.0, 3.0)


def test_one_bar_with_the_seven_notes_of_a_scale_and_one_with_all_twelve_classes():
    scale = [note(120 * i, p) for i, p in enumerate((60, 62, 64, 65, 67, 69, 71))]
    counts, ent, _, _ = counts_of(scale, max_bars=1)
    assert counts[:6] == [7, 0, 1, 1, 7, 7] and abs(float(ent[0]) - math.log2(7)) <= bound([1] * 7 + [0] * 5)
    chromatic = [note(120 * i, 48 + i) for i in range(12)]
    counts, ent, bars, _ = counts_of(chromatic, max_bars=1)
    assert counts[:9] == [12, 0, 1, 1, 12, 12, 48, 59, 12] and bars[0][4:] == [1] * 12
    assert abs(float(ent[0]) - LOG2_12) <= bound([1] * 12) and float(ent[0]) <= LOG2_12 + bound([1] * 12)


def test_four_identical_bars():
    piece = [note(1920 * k + s, p) for k in range(4) for s, p in ((0, 60), (480, 67))]
    counts, ent, bars, _ = counts_of(piece, max_bars=4)
    c = named(counts)
    assert (c["bars_used"], c["pairs"], c["diff"], c["windows_1"], c["windows_4"]) == (4, 6, 0, 4, 1) and sr.gs(counts) == 1.0
    # two classes, one note each: (T[2] - 0) / 2 = 1 exactly; the window of four: (T[8] - (T[4] + T[4])) / 8 = (24 - 16) / 8 = 1 exactly
    assert float(ent[0]) == 4.0 and float(ent[1]) == 1.0
    r = ratios_of((counts, ent))
    assert r["gs"] == 1.0 and r["h1"] == r["h4"] == 1.0 and all(b == bars[0] for b in bars)


def test_two_bars_with_complementary_onset_masks():
    piece = [note(120 * s, 60) for s in range(0, 16, 2)] + [note(1920 + 120 * s, 60) for s in range(1, 16, 2)]
    counts, ent, bars, _ = counts_of(piece, max_bars=2)
    c = named(counts)
    assert bars[0][1] == 0x5555 and bars[1][1] == 0xAAAA and (c["pairs"], c["diff"], c["slots_per_bar"], c["onsets"]) == (1, 16, 16, 16)
    assert sr.gs(counts) == 0.0 and ratios_of((counts, ent))["gs"] == 0.0


def test_an_empty_bar_between_two_full_ones():
    piece = [note(0, 60), note(480, 64), note(2 * 1920, 60), note(2 * 1920 + 480, 64)]
    counts, ent, bars, _ = counts_of(piece, max_bars=5)
    c = named(counts)
    assert (c["bars_used"], c["bars_with_notes"], c["pairs"], c["windows_1"], c["windows_4"]) == (3, 2, 3, 2, 0), "shorter than four bars: no 4-bar window"
    assert c["diff"] == 0 + 2 + 2 and bars[1] == [0, 0, -1, -1] + [0] * 12 and bars[3] == bars[1]
    assert sr.gs(counts) == 1.0 - 4 / 48
    r = ratios_of((counts, ent))
    assert r["empty_bars"] == 1 - 2 / 3 and r["notes_per_bar"] == 2.0 and r["bars"] == 3 and math.isnan(r["h4"])


def test_four_bar_windows_slide_by_one_bar_and_skip_the_empty_ones():
    # bars 0 and 9 hold notes: windows 0 (bars 0..3) and 6 (bars 6..9) are the only ones of 0..6 with a note
    piece = [note(0, 60), note(0, 61), note(9 * 1920, 62)]
    counts, ent, _, _ = counts_of(piece, max_bars=16)
    c = named(counts)
    assert (c["bars_used"], c["windows_1"], c["windows_4"], c["pairs"]) == (10, 2, 2, 45)
    assert float(ent[0]) == 1.0 and float(ent[1]) == 1.0                            # one bit for bar 0 and window 0, none for the others
    # five full bars: windows 0 and 1
    counts = counts_of([note(1920 * k, 60 + k) for k in range(5)], max_bars=8)[0]
    assert named(counts)["windows_4"] == 2 and named(counts)["windows_1"] == 5


@pytest.mark.parametrize("ts", [627, 628, 629, 630])
def test_slot_and_bar_seams(ts):
    tpb = sr.TICKS_PER_BAR[ts]
    Q = tpb // 120
    assert Q in (16, 12, 24)
    for k in (1, 2):
        counts, _, bars, st = counts_of([note(k * tpb + 119, 60), note(k * tpb + 120, 61), note(k * tpb - 1, 62)], meta=meta_of(ts), max_bars=4)
        assert st == sr.OK and counts[11] == Q and counts[0] == 3 and counts[2] == k + 1
        assert bars[k][:2] == [2, 0b11] and bars[k - 1][:2] == [1, 1 << (Q - 1)], (ts, k)
        assert bars[k - 1][2:4] == [62, 62] and bars[k][2:4] == [60, 61]
    # the last tick of the table and the first one behind it
    counts, _, bars, _ = counts_of([note(4 * tpb - 1, 60), note(4 * tpb, 60)], meta=meta_of(ts), max_bars=4)
    assert counts[:3] == [1, 1, 4] and bars[3][:2] == [1, 1 << (Q - 1)]


def test_skipped_notes():
    piece = [note(-1, 60), note(-2 ** 31, 60), note(2 * 1920, 60), note(2 ** 31 - 1, 60), note(0, -1), note(0, 128), note(0, 2 ** 31 - 1),
             note(0, -2 ** 31), note(0, 0), note(1920, 127)]
    counts, ent, bars, st = counts_of(piece, max_bars=2)
    assert st == sr.OK and counts[:8] == [2, 8, 2, 2, 2, 2, 0, 127] and [b[0] for b in bars] == [1, 1]
    assert counts_of(piece, max_bars=3)[0][:3] == [3, 7, 3]                        # bar 2 is inside a table of three
    nothing = counts_of(piece[:2] + piece[4:8], max_bars=2)
    assert nothing[0] == [0, 6, 0, 0, 0, 0, -1, -1, 0, 0, 0, 16, 0, 0, 0, 0] and nothing[1] == (0.0, 0.0) and nothing[3] == sr.OK
    assert counts_of([], max_bars=1)[0] == [0, 0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 16, 0, 0, 0, 0]
    r = ratios_of(nothing[:2])
    assert r["rows"] == 1 and r["notes"] == 0 and r["skipped"] == 6 and all(math.isnan(r[k]) for k in evaluation.StructureTotals.RATIO_NAMES)


def test_every_status():
    n = [note(0, 60), note(10, 62)]
    zero = ([0] * 16, (0.0, 0.0), [[0] * 16])
    assert counts_of(n, valid=False, max_bars=1) == zero + (sr.MASKED,)
    for meta in (META[:1] + [601] + META[2:], META[:1] + [626] + META[2:], meta_of(626), meta_of(631)):
        assert counts_of(n, meta=meta, max_bars=1) == zero + (sr.BAD_META,)
    for kw in (dict(n=-1), dict(n=3), dict(n=2, max_notes=1)):
        assert counts_of(n, max_bars=1, **kw) == zero + (sr.BAD_COUNTS,)
    assert counts_of(n, valid=False, meta=[0] * 11, n=-1)[3] == sr.MASKED          # the order of the table
    assert counts_of(n, meta=[0] * 11, n=-1)[3] == sr.BAD_META
    assert counts_of(n, n=1, max_bars=1)[0][:2] == [1, 0]                          # the count, not the list, says how many notes there are


# ------------------------------------------------------------------------------------------------------------------ the arithmetic
def test_the_table_route_stays_within_its_bound_of_the_direct_formula():
    g = np.random.default_rng(3)
    worst, seen = 0.0, 0
    hists = []
    for _ in range(12000):                                            # random: any number of classes, any size up to the capacity
        N = int(g.integers(1, 32769))
        k = int(g.integers(1, 13))
        cuts = np.sort(g.integers(0, N + 1, size=k - 1))
        parts = np.diff(np.concatenate([[0], cuts, [N]])).tolist() + [0] * (12 - k)
        g.shuffle(parts)
        hists.append([int(x) for x in parts])
    for _ in range(8000):                                             # near-degenerate: almost everything in one class
        N = int(g.integers(2, 32769))
        few = g.integers(0, 3, size=11).tolist()
        rest = N - sum(few)
        if rest < 0:
            few, rest = [0] * 11, N
        parts = few + [rest]
        g.shuffle(parts)
        hists.append([int(x) for x in parts])
    hists += [[32768] + [0] * 11, [32767, 1] + [0] * 10, [2731] * 11 + [2727], [1] * 12, [1] + [0] * 11]
    for h in hists:
        H = float(sr.entropy(h, TABLE))
        err, bd = abs(H - direct(h)), bound(h)
        assert err <= bd and -bd <= H <= LOG2_12 + bd, (h, H, direct(h), bd)
        worst = max(worst, err / bd)
        seen += 1
    assert seen == 20005 and worst < 1.0


def test_the_reference_s_recorded_notes():
    checked = windows = pairs = 0
    for c in fixture_cases():
        if c.status[False] != dr.OK:
            continue
        tpb = sr.TICKS_PER_BAR[int(c.meta[2])]
        max_bars = 1 + max([int(n[0]) // tpb for n in c.notes if n[0] >= 0], default=0)
        counts, ent, bars, st = sr.row_counts(c.notes.tolist(), c.meta, TABLE, max_bars=max_bars)
        d = named(counts)
        assert st == sr.OK and d["notes"] + d["skipped"] == len(c.notes) and d["skipped"] == 0 and d["bars_used"] == (max_bars if len(c.notes) else 0), c.name
        assert sum(b[0] for b in bars) == d["notes"] and d["windows_1"] == d["bars_with_notes"] and d["slots_per_bar"] == tpb // 120
        for b in bars:
            if b[0]:
                H = float(sr.entropy(b[4:], TABLE))
                assert 0.0 <= H <= LOG2_12 and b[2] <= b[3] and 1 <= bin(b[1]).count("1") <= min(b[0], tpb // 120) and b[1] < 1 << (tpb // 120)
        if d["windows_1"]:
            assert 0.0 <= float(ent[0]) / d["windows_1"] <= LOG2_12
        if d["windows_4"]:
            assert 0.0 <= float(ent[1]) / d["windows_4"] <= LOG2_12 and d["windows_4"] <= d["bars_used"] - 3
        if d["pairs"]:
            assert 0.0 <= sr.gs(counts) <= 1.0, c.name
            pairs += 1
        # a shorter table skips the notes behind it and nothing else
        if max_bars > 1:
            short = sr.row_counts(c.notes.tolist(), c.meta, TABLE, max_bars=max_bars - 1)
            assert short[0][0] + short[0][1] == len(c.notes) and short[0][1] == bars[-1][0] and short[2] == bars[:-1]
        checked += 1
        windows += d["windows_4"]
    assert checked > 30 and windows > 20 and pairs > 20


# ------------------------------------------------------------------------------------------------------------------ the totals
def test_ratios_and_gap_on_host_vectors():
    ratios = evaluation.StructureTotals.ratios
    assert len(evaluation.StructureTotals.INT_NAMES) == 12 and len(evaluation.StructureTotals.FLOAT_NAMES) == 4
    # 4 rows, 3 with notes; 90 notes, 5 skipped; 40 bars, 30 with notes; pcs 18, distinct 33, range 60, onsets 75; 30 / 20 windows
    host = [4, 3, 90, 5, 40, 30, 18, 33, 60, 75, 30, 20, 45.0, 50.0, 1.5, 2.0]
    r = ratios(host)
    assert r == {"rows": 4, "notes": 90, "skipped": 5, "bars": 40, "h1": 1.5, "h4": 2.5, "gs": 0.75, "notes_per_bar": 3.0, "empty_bars": 0.25,
                 "pitch_classes": 6.0, "pitch_range": 20.0, "distinct_pitches": 11.0, "onsets_per_bar": 2.5}
    assert isinstance(r["rows"], int) and isinstance(r["h1"], float) and set(evaluation.StructureTotals.RATIO_NAMES) < set(r)
    empty = ratios([0] * 16)
    assert empty["rows"] == 0 and all(math.isnan(empty[k]) for k in evaluation.StructureTotals.RATIO_NAMES)
    one_bar = ratios([1, 1, 3, 0, 1, 1, 2, 3, 7, 3, 1, 0, 0.5, 0.0, 0.0, 0.0])     # no 4-bar window, no pair of bars
    assert one_bar["h1"] == 0.5 and math.isnan(one_bar["h4"]) and math.isnan(one_bar["gs"]) and one_bar["empty_bars"] == 0.0
    gap = evaluation.structure_gap(r, ratios([2, 2, 50, 0, 20, 20, 14, 20, 30, 60, 20, 10, 40.0, 30.0, 2.0, 2.0]))
    assert gap == {"h1": 0.5, "h4": 0.5, "gs": 0.25, "notes_per_bar": 0.5, "empty_bars": 0.25, "pitch_classes": 1.0, "pitch_range": 5.0,
                   "distinct_pitches": 1.0, "onsets_per_bar": 0.5}
    assert all(v == 0.0 for v in evaluation.structure_gap(r, dict(r)).values())
    nan_gap = evaluation.structure_gap(r, one_bar)
    assert math.isnan(nan_gap["h4"]) and math.isnan(nan_gap["gs"]) and nan_gap["h1"] == 1.0
    text = evaluation.structure_block(r)
    assert " H1: 1.500000 " in text and " GS: 0.750000 " in text and " Rows: 4 " in text and text.count("\n") == 14
    assert " Rows" not in evaluation.structure_block(gap, "Structure gap") and "Structure gap" in evaluation.structure_block(gap, "Structure gap")
    assert evaluation.structure_report(r) == {"generated": r}
    assert evaluation.structure_report(r, r) == {"generated": r, "reference": r, "gap": evaluation.structure_gap(r, r)}


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    lib = _lib.lib()
    buf = (C.c_int64 * 64)()
    a = C.addressof(buf)
    ok = dict(notes=a, counts3=a, meta=a, valid=a, xlog2x=a, out=a, entropy=a, bars=a, status=a, B=1, max_notes=4, max_bars=1)
    bad = [dict(notes=None), dict(counts3=None), dict(meta=None), dict(xlog2x=None), dict(out=None), dict(entropy=None), dict(status=None),
           dict(B=0), dict(B=-2), dict(max_notes=0), dict(max_notes=-1), dict(max_notes=32769), dict(max_bars=0), dict(max_bars=-1),
           dict(max_bars=513)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhm_structure_counts(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"structure_counts" in lib.mh_last_error()
    assert not any(buf), "a refused call writes nothing"
    # the Python front refuses the same before it touches the library or asks for a device
    import torch
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    for call in (lambda: metric.structure_counts_raw(z(1, 4, 4), z(1, 3), z(1, 11), max_bars=0),
                 lambda: metric.structure_counts_raw(z(1, 4, 4), z(1, 3), z(1, 11), max_bars=513),
                 lambda: metric.structure_counts_raw(z(1, 4, 3), z(1, 3), z(1, 11)),
                 lambda: metric.structure_counts_raw(z(1, 4), z(1, 3), z(1, 11)),
                 lambda: metric.structure_counts_raw(z(1, 4, 4), z(1, 2), z(1, 11)),
                 lambda: metric.structure_counts_raw(z(1, 4, 4), z(1, 3), z(2, 11)),
                 lambda: metric.structure_counts_raw(z(1, 32769, 4), z(1, 3), z(1, 11)),
                 lambda: metric.structure_counts_raw(z(0, 4, 4), z(0, 3), z(0, 11))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.MuseHipError):
        metric.structure_counts_raw(z(1, 4, 4), z(1, 3), z(1, 11))                 # host tensors: there is no CPU path
