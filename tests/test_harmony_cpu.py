"""CPU: the chord-fit rule without a device.  tests/harmony_ref.py (the plain-Python restatement of csrc/harmony.hip) against music -
every chord token and every key spelled by note names -, on hand-made rows with answers worked out here, on every record of
tests/golden/decode.npz (the reference's own recorded notes and markers against the decode restatement's), the bar a note starts in
against the bar ordinal an infill plan gives its tokens;
the refusals of the entry point, which come before any launch.  No kernel runs here: the device side is tests/test_harmony_gpu.py and
tests/test_harmony_sampling_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as dr
import harmony_ref as hr
import infill_ref as ir
from musediffusion_amd import _lib, metric
from musediffusion_amd.utils import decode_util as du
from test_decode_cpu import fixture_cases

CHROMATIC = ("c", "c#", "d", "d#", "e", "f", "f#", "g", "g#", "a", "a#", "b")
# a quality spelled as the intervals a musician names
SEMITONES = {"root": 0, "minor third": 3, "major third": 4, "perfect fourth": 5, "diminished fifth": 6, "perfect fifth": 7,
             "augmented fifth": 8, "minor seventh": 10, "major seventh": 11}
QUALITY = {"": ("root", "major third", "perfect fifth"),
           "7": ("root", "major third", "perfect fifth", "minor seventh"),
           "+": ("root", "major third", "augmented fifth"),
           "dim": ("root", "minor third", "diminished fifth"),
           "m": ("root", "minor third", "perfect fifth"),
           "m7": ("root", "minor third", "perfect fifth", "minor seventh"),
           "m7b5": ("root", "minor third", "diminished fifth", "minor seventh"),
           "maj7": ("root", "major third", "perfect fifth", "major seventh"),
           "sus4": ("root", "perfect fourth", "perfect fifth")}
SHARP_OF = {"db": "c#", "eb": "d#", "gb": "f#", "ab": "g#", "bb": "a#"}
WHOLE, HALF = 2, 1
STEPS = {"major": (WHOLE, WHOLE, HALF, WHOLE, WHOLE, WHOLE), "minor": (WHOLE, HALF, WHOLE, WHOLE, HALF, WHOLE)}

META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]   # c major, 4/4: 1920 ticks a bar
CHORD = lambda name: 195 + du.CHORD_NAMES.index(name)  # noqa: E731


def spell(name):
    """'f#m7b5' -> {'f#', 'a', 'c', 'e'}"""
    root = name[:2] if name[:2] in CHROMATIC else name[:1]
    at = CHROMATIC.index(root)
    return {CHROMATIC[(at + SEMITONES[i]) % 12] for i in QUALITY[name[len(root):]]}


def names(pcs):
    return {CHROMATIC[p] for p in pcs}


def note(start, pitch, length=100, velocity=64):
    return (start, start + length, pitch, velocity)


def counts_of(notes, chords, meta=META, **kw):
    return hr.row_counts(notes, chords, meta, **kw)


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_every_chord_token_spells_its_tones_by_name():
    assert len(du.CHORD_NAMES) == 109 and du.CHORD_NAMES[0] == "a" and du.CHORD_NAMES[108] == "NN"
    for token in range(195, 303):
        assert names(hr.chord_tones(token)) == spell(du.CHORD_NAMES[token - 195]), (token, du.CHORD_NAMES[token - 195])
    by_hand = {"am7": "a c e g", "c": "c e g", "f#m7b5": "f# a c e", "g#+": "g# c e", "g7": "g b d f", "bdim": "b d f", "dsus4": "d g a",
               "fmaj7": "f a c e", "a#m": "a# c# f", "em7": "e g b d", "d#": "d# g a#"}
    for name, tones in by_hand.items():
        assert names(hr.chord_tones(CHORD(name))) == set(tones.split()) == spell(name), name
    for token in (303, 304, 194, 0, -1, 2 ** 31 - 1, -2 ** 31):
        assert hr.chord_tones(token) is None


def test_every_key_spells_its_scale_by_name():
    assert len(du.KEY_NAMES) == 24 and du.KEY_NAMES[0] == "cmajor" and du.KEY_NAMES[21] == "aminor"
    for token in range(602, 626):
        name = du.KEY_NAMES[token - 602]
        mode = name[-5:]
        root = SHARP_OF.get(name[:-5], name[:-5])
        at, scale = CHROMATIC.index(root), {root}
        for step in STEPS[mode]:
            at = (at + step) % 12
            scale.add(CHROMATIC[at])
        assert len(scale) == 7 and names(hr.scale_tones(token)) == scale, name
    white = set("c d e f g a b".split())
    assert names(hr.scale_tones(602)) == white and names(hr.scale_tones(623)) == white          # c major and a minor
    assert names(hr.scale_tones(609)) == set("g a b c d e f#".split())                           # g major
    assert names(hr.scale_tones(614)) == set("c d d# f g g# a#".split())                         # c minor
    assert hr.TICKS_PER_BAR == {627 + i: 480 * dr.BEATS[i] for i in range(4)}


def test_status_codes_mirror_the_header():
    assert (hr.OK, hr.MASKED, hr.BAD_META, hr.BAD_COUNTS) == tuple(range(4))
    assert _lib.ABI["musehip_harmony.h"].enums == {"MHH_OK": 0, "MHH_MASKED": 1, "MHH_BAD_META": 2, "MHH_BAD_COUNTS": 3}
    assert (metric.HARMONY_OK, metric.HARMONY_MASKED, metric.HARMONY_BAD_META, metric.HARMONY_BAD_COUNTS) == tuple(range(4))
    assert len(metric.HARMONY_COUNT_NAMES) == 8


# ------------------------------------------------------------------------------------------------------------------ hand-made rows
def test_arpeggio_under_its_chord_and_under_the_chord_a_semitone_up():
    arp = [note(0, 60, 100), note(480, 64, 200), note(960, 67, 300), note(1440, 72, 400)]      # c e g c
    counts, hist, bars, st = counts_of(arp, [(0, CHORD("c"))], max_bars=2)
    assert st == hr.OK and counts == [4, 4, 4, 4, 1000, 1000, 1000, 1]
    assert hist == [2, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0] and bars == [[4, 4, 4, 4], [0, 0, 0, 0]]
    counts, hist, bars, st = counts_of(arp, [(0, CHORD("c#"))], max_bars=1)                   # c# f g#: none of c e g
    assert counts == [4, 4, 0, 4, 1000, 1000, 0, 1] and bars == [[4, 4, 0, 4]]
    counts = counts_of(arp, [(0, CHORD("c#"))], meta=META[:1] + [603] + META[2:])[0]            # db major: only c is in the scale
    assert counts[:4] == [4, 4, 0, 2]
    counts = counts_of(arp, [(0, CHORD("am7"))])[0]                                            # a c e g holds all of c e g
    assert counts[:3] == [4, 4, 4]


def test_a_chord_at_the_onset_is_in_force_and_one_tick_later_is_not():
    n = [note(1000, 61)]                                                                        # c#: in c#, not in c
    assert counts_of(n, [(0, CHORD("c")), (1000, CHORD("c#"))])[0][:3] == [1, 1, 1]
    assert counts_of(n, [(0, CHORD("c")), (1001, CHORD("c#"))])[0][:3] == [1, 1, 0]
    assert counts_of(n, [(0, CHORD("c")), (999, CHORD("c#"))])[0][:3] == [1, 1, 1]
    # the chord at the onset judges the whole note: the change at 1001 does not split a note that sounds until 1100
    assert counts_of([note(1000, 61, 100)], [(1000, CHORD("c#")), (1001, CHORD("c"))])[0] == [1, 1, 1, 0, 100, 100, 100, 1]


def test_notes_no_chord_judges():
    early = [note(10, 60), note(20, 64)]
    assert counts_of(early, [(11, CHORD("c"))])[0][:4] == [2, 1, 1, 2]                          # the first starts before the first chord
    assert counts_of(early, [])[0][:4] == [2, 0, 0, 2]
    assert counts_of(early, [(0, 303)])[0][:4] == [2, 0, 0, 2]                                  # Chord_NN
    assert counts_of(early, [(0, 304)])[0][:4] == [2, 0, 0, 2]                                  # no chord token at all
    assert counts_of(early, [(0, CHORD("c")), (15, 303)])[0] == [2, 1, 1, 2, 200, 100, 100, 1]  # NN in force silences the chord before it
    assert counts_of([note(-5, 60)], [(-5, CHORD("c"))], max_bars=1)[:3] == ([1, 1, 1, 1, 100, 100, 100, 0], [1] + [0] * 11, [[0] * 4])


def test_equal_ticks_take_the_last_entry_and_order_does_not_matter():
    n = [note(500, 61), note(2000, 60)]
    assert counts_of(n, [(0, CHORD("c#")), (0, CHORD("c"))])[0][:3] == [2, 2, 1]                # c in force: 61 off, 60 on
    assert counts_of(n, [(0, CHORD("c")), (0, CHORD("c#"))])[0][:3] == [2, 2, 1]                # c# in force: 61 on, 60 off
    assert counts_of(n, [(0, CHORD("c")), (0, CHORD("c#")), (0, CHORD("c"))])[0][:3] == [2, 2, 1]
    g = np.random.default_rng(7)
    for _ in range(50):
        chords = [(int(g.integers(0, 12)) * 240, int(g.integers(190, 306))) for _ in range(int(g.integers(1, 12)))]
        g.shuffle(chords)
        notes = [note(int(g.integers(-100, 3000)), int(g.integers(0, 128)), int(g.integers(-50, 900))) for _ in range(20)]
        stable = sorted(chords, key=lambda c: c[0])                                             # Python's sort is stable
        assert counts_of(notes, chords, max_bars=3) == counts_of(notes, stable, max_bars=3)


def test_lengths_pitch_classes_bars_and_statuses():
    n = [(0, 70000, 60, 1), (100, 50, 61, 1), (5000, 5001, -1, 1), (-1, 3, 128, 1), (3840, 3841, -2 ** 31, 1)]
    counts, hist, bars, st = counts_of(n, [(0, CHORD("c"))], max_bars=2)
    # lengths 65535, 0, 1, 4, 1; pitch classes 0, 1, 11, 8, 4; the note at -1 is before the chord; bars 0, 0, 2, -, 2
    assert counts == [5, 4, 2, 3, 65541, 65537, 65536, 3]
    assert hist == [1, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1] and bars == [[2, 2, 1, 1], [0, 0, 0, 0]]
    assert counts_of(n, [(0, CHORD("c"))], max_bars=3)[2][2] == [2, 2, 1, 2]
    zero = ([0] * 8, [0] * 12, [[0] * 4])
    assert counts_of(n, [], valid=False, max_bars=1) == zero + (hr.MASKED,)
    for meta in (META[:1] + [601] + META[2:], META[:1] + [626] + META[2:], META[:2] + [626] + META[3:], META[:2] + [631] + META[3:]):
        assert counts_of(n, [], meta=meta, max_bars=1) == zero + (hr.BAD_META,)
    for kw in (dict(n=-1), dict(n=6), dict(c=-1), dict(c=1)):
        assert counts_of(n, [], max_bars=1, **kw) == zero + (hr.BAD_COUNTS,)
    assert counts_of(n, [], valid=False, meta=[0] * 11, n=-1)[3] == hr.MASKED                   # the order of the table
    assert counts_of(n, [], meta=[0] * 11, n=-1)[3] == hr.BAD_META
    for ts, tpb in ((627, 1920), (628, 1440), (629, 1440), (630, 2880)):
        assert counts_of([note(tpb - 1, 60), note(tpb, 60)], [], meta=META[:2] + [ts] + META[3:], max_bars=2)[2] == [[1, 0, 0, 1], [1, 0, 0, 1]]


# ------------------------------------------------------------------------------------------------------------------ the fixture
def _decoded_ok():
    """(case, strict, decode restatement's row) of every record and validation mode that decodes"""
    out = []
    for c in fixture_cases():
        for strict in (False, True):
            if c.status[strict] == dr.OK:
                out.append((c, strict, dr.decode_row(c.tokens, c.mask, dr.MAX_ROW, 2048, 2048, strict)))
    return out


def test_the_reference_s_recorded_notes_and_markers_give_what_the_decode_restatement_s_give():
    checked = judged_total = 0
    for c, strict, r in _decoded_ok():
        assert r["status"] == dr.OK, c.name
        recorded = [(int(t), CHORD(name)) for t, name in zip(c.marker_time, c.marker_text)]
        want = hr.row_counts(c.notes.tolist(), recorded, c.meta, max_bars=hr_max_bars(c.notes, c.meta))
        got = hr.row_counts(r["notes"].tolist(), r["chords"].tolist(), r["meta"], max_bars=hr_max_bars(c.notes, c.meta))
        assert got == want and got[3] == hr.OK, c.name
        counts, hist, bars, _ = got
        scale = hr.scale_tones(c.meta[1])
        under_nn = before = 0
        for n in c.notes.tolist():
            at = hr.chord_in_force(recorded, n[0])
            before += at < 0
            under_nn += at >= 0 and hr.chord_tones(recorded[at][1]) is None
        assert counts[0] == len(c.notes) == counts[1] + under_nn + before == sum(hist), c.name
        assert counts[3] == sum(1 for n in c.notes.tolist() if n[2] % 12 in scale), c.name
        assert len(bars) >= counts[7] and [sum(b[i] for b in bars) for i in range(4)] == counts[:4], c.name
        checked += 1
        judged_total += counts[1]
    assert checked > 60 and judged_total > 300


def hr_max_bars(notes, meta):
    tpb = hr.TICKS_PER_BAR[int(meta[2])]
    return 1 + max([int(n[0]) // tpb for n in notes if n[0] >= 0], default=0)


def first_bar_shift(restored):
    """1 when the first token the decoder keeps (2..559) is not BAR: the decoder then counts the notes in front of the first BAR as bar 0
    and the first BAR opens bar 1"""
    kept = [int(t) for t in restored if 2 <= int(t) <= 559]
    return 0 if kept[:1] == [ir.BAR] else 1


def test_a_note_starts_in_the_bar_an_infill_plan_gives_its_tokens():
    """start / ticks_per_bar of every decoded note is the bar ordinal of tests/infill_ref.py's layout for the note's tokens, so
    run_infill may hand its `bars` to HarmonyTotals.  The one quirk (zero records disagree once it is applied): a note region that does
    not begin with BAR - the decoder opens bar 1 at the first BAR, the plan bar 0, and the notes in front of it are bar 0 to the
    decoder and no bar (-1) to the plan; evaluation.HarmonyTotals adds the same shift."""
    checked, shifted, disagree = 0, set(), []
    for c, strict, r in _decoded_ok():
        toks, mask = [int(t) for t in c.tokens], [int(t) for t in c.mask]
        st, m, e, _ = ir.layout(toks, mask)
        assert st == ir.OK, c.name
        tpb = hr.TICKS_PER_BAR[int(r["meta"][2])]
        kept, k = [], -1                                            # the tokens the decoder keeps, each with the plan's bar ordinal
        for j in range(m, e):
            k += toks[j] == ir.BAR
            if 2 <= toks[j] <= 559:
                kept.append((toks[j], k))
        quads = {(kept[i][1], kept[i][0] - 432, kept[i + 2][0] - 3) for i in range(len(kept) - 3)
                 if [ir.token_class(t) for t, _ in kept[i:i + 4]] == [0, 1, 2, 3]}
        shift = first_bar_shift(r["restored"])
        if shift:
            shifted.add(c.name)
        for n in r["notes"].tolist():
            bar = n[0] // tpb
            position = [p for p in range(128) if p * tpb // 128 == n[0] - bar * tpb]
            assert len(position) == 1
            if (bar - shift, position[0], n[2]) not in quads:
                disagree.append((c.name, strict, n))
            checked += 1
    assert checked > 300 and not disagree, disagree[:5]
    assert shifted == {"branch_fewer_by_one_no_bar", "first_token_is_a_note", "gen_shift_mask_1", "mask_one_long"}


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    lib = _lib.lib()
    buf = (C.c_int32 * 64)()
    a = C.addressof(buf)
    ok = dict(notes=a, chords=a, counts3=a, meta=a, valid=a, out=a, hist=a, bars=a, status=a, B=1, max_notes=4, max_chords=4, max_bars=1)
    bad = [dict(notes=None), dict(chords=None), dict(counts3=None), dict(meta=None), dict(out=None), dict(status=None), dict(B=0), dict(B=-2),
           dict(max_notes=0), dict(max_notes=-1), dict(max_notes=32769), dict(max_chords=0), dict(max_chords=4097), dict(max_bars=-1),
           dict(max_bars=513), dict(bars=None), dict(max_bars=0), dict(bars=None, max_bars=512)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhh_harmony_counts(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"harmony_counts" in lib.mh_last_error()
    # the Python front refuses the same before it touches the library
    import torch
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    with pytest.raises(_lib.MuseHipError):
        metric.harmony_counts_raw(z(1, 4, 4), z(1, 4, 2), z(1, 3), z(1, 11))                   # host tensors: there is no CPU path
