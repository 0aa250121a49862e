"""CPU: the interplay rule and the song utilities without a device.  tests/interplay_ref.py (the plain-Python restatement of
csrc/arrange.hip) on hand-made songs with answers worked out here, on every status, and the identities that hold per song;
utils.arrange_util.align_shift on host tensors, write_song read back by read_song and by read_midi; evaluation.InterplayTotals.ratios
on host vectors; the refusals of the entry point, which
come before any launch.  No kernel runs here: the device side is tests/test_interplay_gpu.py and tests/test_arrange_sampling_gpu.py."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import interplay_ref as ir
from musediffusion_amd import _lib, evaluation, metric
from musediffusion_amd.utils import arrange_util as au, decode_util as du

META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]   # 100 bpm, c major, 4/4


def song_of(*rows, metas=None, **kw):
    """rows: lists of (start, end, pitch, velocity) -> interplay_ref.batch_counts of ONE song holding them"""
    cap = max(1, max(len(r) for r in rows))
    notes = np.zeros((len(rows), cap, 4), np.int32)
    for b, r in enumerate(rows):
        notes[b, :len(r)] = np.array(r, np.int64).reshape(-1, 4)
    counts3 = np.array([[len(r), 0, 0] for r in rows], np.int32)
    meta = np.array(metas if metas is not None else [META] * len(rows), np.int32)
    return ir.batch_counts(notes, counts3, meta, **kw)


def test_names_and_status_codes_mirror_the_header():
    assert (ir.OK, ir.MASKED, ir.BAD_COUNTS, ir.BAD_SHIFT, ir.MIXED) == tuple(range(5))
    assert _lib.ABI["musehip_arrange.h"].enums == {"MHA_OK": 0, "MHA_MASKED": 1, "MHA_BAD_COUNTS": 2, "MHA_BAD_SHIFT": 3, "MHA_MIXED": 4}
    assert (metric.INTERPLAY_OK, metric.INTERPLAY_MASKED, metric.INTERPLAY_BAD_COUNTS, metric.INTERPLAY_BAD_SHIFT,
            metric.INTERPLAY_MIXED) == tuple(range(5))
    assert len(metric.INTERPLAY_COUNT_NAMES) == 8 and len(metric.INTERPLAY_COLUMN_NAMES) == 9
    assert (metric.INTERPLAY_MAX_NOTES, metric.INTERPLAY_MAX_SHIFT, metric.DRUMS_INST) == (32768, 2 ** 29, 648) == (32768, ir.MAX_TICK, ir.DRUMS)
    assert ir.TICKS_PER_BAR == {627 + i: 480 * b for i, b in enumerate((4, 3, 3, 6))}


# ------------------------------------------------------------------------------------------------------------------ hand-made songs
def test_a_fifth_overlapping_240_ticks():
    out = song_of([(0, 480, 60, 90)], [(240, 960, 67, 90)])              # c4 under g4: d = 7, class 5; common ticks 480 - 240
    assert out["status"].tolist() == [0, 0]
    assert out["pairs"].tolist() == [[0, 0, 0, 0, 0, 1, 0, 1, 0], [0, 0, 0, 0, 0, 1, 0, 0, 1]]
    assert out["ticks"].tolist() == [[0, 0, 0, 0, 0, 240, 0, 240, 0], [0, 0, 0, 0, 0, 240, 0, 0, 240]]
    assert out["counts"].tolist() == [[1, 0, 1, 1, 0, 0, 0, 0]] * 2


def test_a_tritone_an_octave_and_identical_notes():
    out = song_of([(0, 100, 60, 1)], [(0, 100, 66, 1)])                  # the tritone is its own inversion: class 6
    assert out["pairs"][:, 6].tolist() == [1, 1] and out["ticks"][:, 6].tolist() == [100, 100] and out["pairs"][:, :6].sum() == 0
    out = song_of([(0, 100, 48, 1)], [(50, 100, 72, 1)])                 # two octaves: class 0, and the rows are below / above
    assert out["pairs"].tolist() == [[1, 0, 0, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 0, 0, 0, 1]] and out["ticks"][:, 0].tolist() == [50, 50]
    out = song_of([(0, 100, 60, 1)], [(0, 100, 60, 9)])                  # the same note twice: class 0, neither below nor above
    assert out["pairs"].tolist() == [[1] + [0] * 8] * 2 and out["ticks"].tolist() == [[100] + [0] * 8] * 2
    out = song_of([(0, 10, 0, 1)], [(0, 10, 127, 1)])                    # d = 127 mod 12 = 7 -> class 5
    assert out["pairs"][0].tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 0]
    for d, ic in enumerate([0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1, 0, 1]):
        out = song_of([(0, 10, 50, 1)], [(0, 10, 50 + d, 1)])
        assert out["pairs"][0, :7].tolist() == [int(c == ic) for c in range(7)], d


def test_touching_notes_do_not_sound_together():
    out = song_of([(0, 480, 60, 1), (960, 1000, 60, 1)], [(480, 960, 64, 1)])
    assert not out["pairs"].any() and not out["ticks"].any()
    assert out["counts"].tolist() == [[2, 0, 1, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 0]]
    out = song_of([(0, 481, 60, 1), (959, 1000, 60, 1)], [(480, 960, 64, 1)])   # one tick each
    assert out["pairs"][:, 4].tolist() == [2, 2] and out["ticks"][:, 4].tolist() == [2, 2] and out["counts"][:, 3].tolist() == [2, 1]


def test_the_clamp_at_65535_ticks_a_pair():
    out = song_of([(0, 65535, 60, 1)], [(0, 70000, 61, 1)])
    assert out["ticks"][0, 1] == 65535 and out["ticks"][0, 7] == 65535
    out = song_of([(0, 65536, 60, 1), (0, 2 ** 29, 60, 1)], [(0, 2 ** 29, 61, 1)])
    assert out["ticks"][0].tolist() == [0, 2 * 65535, 0, 0, 0, 0, 0, 2 * 65535, 0] and out["pairs"][1, 1] == 2


def test_shifts_move_a_row_and_skipped_notes_count_as_such():
    rows = ([(0, 100, 60, 1)], [(0, 100, 64, 1)])
    assert song_of(*rows, shift=[0, 100])["pairs"].sum() == 0
    out = song_of(*rows, shift=[50, 100])
    assert out["ticks"][0].tolist() == [0, 0, 0, 0, 50, 0, 0, 50, 0]
    assert song_of(*rows, shift=[2 ** 29, 2 ** 29])["ticks"][0, 4] == 100
    bad = [(-1, 100, 60, 1), (0, 100, -1, 1), (0, 100, 128, 1), (100, 100, 60, 1), (100, 50, 60, 1), (0, 2 ** 29 + 1, 60, 1), (5, 95, 60, 1)]
    out = song_of(bad, [(0, 100, 64, 1)])
    assert out["counts"].tolist() == [[1, 6, 1, 1, 0, 0, 0, 0], [1, 0, 1, 1, 0, 0, 0, 0]]
    assert out["pairs"][:, 4].tolist() == [1, 1] and out["ticks"][:, 4].tolist() == [90, 90]


def test_every_status():
    a, b = [(0, 100, 60, 1)], [(0, 100, 64, 1)]
    out = song_of(a, b, a, valid=[1, 0, 1])
    assert out["status"].tolist() == [0, ir.MASKED, 0] and out["counts"][:, 2].tolist() == [1, 0, 1] and not out["pairs"][1].any()
    assert out["pairs"][0].tolist() == [1] + [0] * 8, "a masked row is nobody's partner"
    out = song_of(a, b, shift=[0, -1])
    assert out["status"].tolist() == [0, ir.BAD_SHIFT] and out["counts"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert song_of(a, b, shift=[2 ** 29 + 1, 0])["status"].tolist() == [ir.BAD_SHIFT, 0]
    notes = np.zeros((3, 2, 4), np.int32)
    notes[:, 0] = (0, 100, 60, 1)
    meta = np.array([META] * 3, np.int32)
    out = ir.batch_counts(notes, np.array([[1, 0, 0], [3, 0, 0], [-1, 0, 0]], np.int32), meta)
    assert out["status"].tolist() == [0, ir.BAD_COUNTS, ir.BAD_COUNTS] and out["counts"][0, 2] == 0
    # the order: MASKED before BAD_COUNTS before BAD_SHIFT before MIXED
    odd = np.array([META, META[:1] + [603] + META[2:]], np.int32)
    out = ir.batch_counts(notes[:2], np.array([[9, 0, 0], [1, 0, 0]], np.int32), odd, valid=[0, 1], shift=[-1, 0])
    assert out["status"].tolist() == [ir.MASKED, 0]
    out = ir.batch_counts(notes[:2], np.array([[9, 0, 0], [1, 0, 0]], np.int32), odd, shift=[-1, 0])
    assert out["status"].tolist() == [ir.BAD_COUNTS, 0]
    out = ir.batch_counts(notes[:2], np.array([[1, 0, 0], [1, 0, 0]], np.int32), odd, shift=[-1, 0])
    assert out["status"].tolist() == [ir.BAD_SHIFT, 0]
    out = ir.batch_counts(notes[:2], np.array([[1, 0, 0], [1, 0, 0]], np.int32), odd)
    assert out["status"].tolist() == [ir.MIXED, ir.MIXED] and not any(out[k].any() for k in ("counts", "pairs", "ticks"))


@pytest.mark.parametrize("field", [0, 1, 2])
def test_one_odd_row_makes_every_row_of_its_song_mixed(field):
    metas = [list(META) for _ in range(4)]
    metas[1][field] += 1
    rows = [[(0, 100, 60 + b, 1)] for b in range(4)]
    out = song_of(*rows, metas=metas, song=[5, 5, 5, -5])
    assert out["status"].tolist() == [ir.MIXED] * 3 + [0] and not out["pairs"].any() and out["counts"][3].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    metas[1][field] -= 1
    metas[1][3 + field] += 1                                             # the other eight fields may differ: the tracks of a song do
    assert song_of(*rows, metas=metas, song=[5, 5, 5, -5])["status"].tolist() == [0] * 4


def test_the_identities_hold_per_song():
    g = np.random.default_rng(3)
    B, cap = 9, 40
    notes = np.zeros((B, cap, 4), np.int32)
    notes[:, :, 0] = g.integers(0, 3000, size=(B, cap))
    notes[:, :, 1] = notes[:, :, 0] + g.integers(1, 700, size=(B, cap))
    notes[:, :, 2] = g.integers(40, 80, size=(B, cap))
    counts3 = np.zeros((B, 3), np.int32)
    counts3[:, 0] = g.integers(20, cap + 1, size=B)
    song = np.array([7, 7, 7, -1, -1, 7, 2 ** 31 - 1, -1, -1], np.int32)
    out = ir.batch_counts(notes, counts3, np.array([META] * B, np.int32), song=song, shift=g.integers(0, 500, size=B))
    assert (out["status"] == 0).all() and out["counts"][:, 2].tolist() == [3, 3, 3, 3, 3, 3, 0, 3, 3]
    for s in (7, -1, 2 ** 31 - 1):
        rows = song == s
        p, t = out["pairs"][rows].sum(0), out["ticks"][rows].sum(0)
        assert (p[:7] % 2 == 0).all() and (t[:7] % 2 == 0).all(), "every pair is seen from both rows"
        assert p[7] == p[8] and t[7] == t[8], "where one row is below the other is above"
        equal_pitch = p[:7].sum() - p[7] - p[8]
        assert equal_pitch >= 0 and equal_pitch % 2 == 0
        assert (out["pairs"][rows][:, 7] + out["pairs"][rows][:, 8] <= out["pairs"][rows][:, :7].sum(1)).all()
    assert out["pairs"][song == 7].sum() > 500 and not out["pairs"][6].any()
    # equal pitches counted directly for one pair of rows
    a, b = [(0, 10, 60, 1), (0, 10, 61, 1)], [(5, 10, 60, 1), (0, 3, 61, 1), (0, 10, 72, 1)]
    out = song_of(a, b)
    p = out["pairs"].sum(0)
    assert p[:7].sum() - p[7] - p[8] == 2 * 2 and p[7] == p[8] == 4


# ------------------------------------------------------------------------------------------------------------------ align_shift
def decoded_of(rows, metas, status=None):
    """host stand-in of a DecodedBatch: rows of restored tokens (zero padded)"""
    L = max(len(r) for r in rows)
    restored = torch.zeros(len(rows), L, dtype=torch.int32)
    for b, r in enumerate(rows):
        restored[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return SimpleNamespace(restored=restored, lengths=torch.tensor([len(r) for r in rows], dtype=torch.int32),
                           meta=torch.tensor(metas, dtype=torch.int32), status=torch.tensor(status or [0] * len(rows), dtype=torch.int32))


def test_align_shift_on_host_tensors():
    bar_first, note_first, chord_first = [2, 140, 300, 60, 400], [140, 300, 60, 400, 2], [600, 700, 2, 140]
    ts = lambda t: META[:2] + [t] + META[3:]  # noqa: E731
    rows = [bar_first, note_first, bar_first, bar_first, bar_first, note_first, bar_first, [], chord_first, note_first]
    metas = [ts(627), ts(627), ts(628), ts(627), ts(630), ts(630), ts(629), ts(627), ts(627), ts(627)]
    song = [0, 0, 0, 1, 2, 2, 2, 0, 3, 3]
    status = [0, 0, 0, 0, 0, 0, 0, 0, 0, du.NO_EOS]
    dec = decoded_of(rows, metas, status)
    f = du.first_bar_shift(dec).tolist()
    assert f == [0, 1, 0, 0, 0, 1, 0, 0, 0, 1] == [ir.first_bar_shift(dec.restored[b].tolist(), len(rows[b])) for b in range(len(rows))]
    assert evaluation._first_bar_shift is du.first_bar_shift
    got = au.align_shift(dec, torch.tensor(song))
    assert got.dtype == torch.int32 and got.tolist() == [1920, 0, 1440, 0, 2880, 0, 1440, 1920, 0, 0]
    assert got.tolist() == ir.align_shift(f, [s == 0 for s in status], song, metas)
    # a late row that did not decode moves nobody (song 3 above); ids are compared, not used as indices
    assert au.align_shift(dec, torch.tensor([-7 if s == 0 else 2 ** 31 - 1 for s in song], dtype=torch.int32)).tolist()[:3] == [1920, 0, 1440]
    assert au.align_shift(decoded_of([bar_first, note_first], [ts(626), ts(627)]), torch.tensor([0, 0])).tolist() == [0, 0], "no bar length for that token"


# ------------------------------------------------------------------------------------------------------------------ song files
def meta_row(inst, role):
    return META[:5] + [inst] + META[6:9] + [role] + META[10:]


def test_write_song_is_read_back_by_read_song_and_read_midi(tmp_path):
    tracks = [np.array([[0, 480, 60, 90], [480, 960, 64, 80], [480, 600, 67, 70]], np.int32), np.array([[0, 1920, 36, 100]], np.int32),
              np.zeros((0, 4), np.int32), np.array([[0, 120, 38, 110], [240, 360, 42, 60]], np.int32),
              np.array([[10, 20, 127, 1]], np.int32), np.array([[0, 240, 35, 99]], np.int32)]
    meta = [meta_row(642, 720), meta_row(645, 723), meta_row(646, 724), meta_row(648, 725), meta_row(641, 719), meta_row(648, 722)]
    chords = np.array([[0, 198], [1920, 250]], np.int32)
    shifts = [0, 1920, 0, 1920, 7, 0]
    path = tmp_path / "song.midi"
    au.write_song(path, tracks, chords, meta, shifts)
    tpb, got = au.read_song(path)
    assert tpb == 480 and len(got) == 6
    assert [g[0] for g in got] == ["main_melody_0", "bass_1", "pad_2", "riff_3", "unknown_4", "accompaniment_5"]
    assert [g[1] for g in got] == [0, 1, 2, 9, 3, 9], "drum rows on channel 9, pitched rows in order"
    assert [g[2] for g in got] == [0, 32, 48, 0, 0, 0]
    for g, notes, s in zip(got, tracks, shifts):
        want = notes.astype(np.int64)
        want[:, :2] += s
        assert g[3].dtype == np.int32 and g[3].tolist() == want[np.argsort(want[:, 0], kind="stable")].tolist()
    # the conductor track is write_midi's, byte for byte, and read_midi returns the first note track
    single = tmp_path / "single.midi"
    du.write_midi(single, tracks[0], chords, meta[0])
    a, b = open(path, "rb").read(), open(single, "rb").read()
    t0 = 22 + int.from_bytes(b[18:22], "big")
    assert a[:10] == b[:10] and a[10:12] == b"\x00\x07" and b[10:12] == b"\x00\x02" and a[12:t0] == b[12:t0]
    assert a[t0:t0 + 4] == b"MTrk" and a[t0 + 8:t0 + 12] == b"\x00\xff\x03\x0d" and a[t0 + 12:t0 + 25] == b"main_melody_0"
    tpb1, first = du.read_midi(path)
    assert tpb1 == 480 and first.tolist() == tracks[0].tolist() == du.read_midi(single)[1].tolist()
    # names of the caller's; every program of the table; a bass role on another group keeps the group's program
    au.write_song(path, tracks[:2], chords, meta[:2], [0, 0], names=["lead", "low"])
    assert [g[0] for g in au.read_song(path)[1]] == ["lead", "low"]
    insts = list(range(641, 651))
    au.write_song(path, [tracks[4]] * 10, chords, [meta_row(i, 723) for i in insts], [0] * 10)
    got = au.read_song(path)[1]
    assert [g[2] for g in got] == [0, 0, 21, 11, 32, 48, 61, 0, 52, 54] and [g[1] for g in got] == [0, 1, 2, 3, 4, 5, 6, 9, 7, 8]
    assert au.track_program(meta_row(645, 722)) == (24, False) and au.track_program(meta_row(648, 723)) == (0, True)


def test_fifteen_pitched_tracks_fit_and_the_sixteenth_raises(tmp_path):
    one = np.array([[0, 10, 60, 1]], np.int32)
    chords = np.zeros((0, 2), np.int32)
    metas = [meta_row(642, 720)] * 15 + [meta_row(648, 720)] * 2
    au.write_song(tmp_path / "full.midi", [one] * 17, chords, metas, [0] * 17)
    got = au.read_song(tmp_path / "full.midi")[1]
    assert [g[1] for g in got] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 9, 9]
    with pytest.raises(ValueError, match="16 pitched"):
        au.write_song(tmp_path / "over.midi", [one] * 16, chords, [meta_row(642, 720)] * 16, [0] * 16)
    assert not (tmp_path / "over.midi").exists()
    for bad in (dict(shifts=[0]), dict(names=["a"]), dict(tracks=[])):
        args = dict(tracks=[one] * 2, chords=chords, meta=metas[:2], shifts=[0, 0], names=None)
        args.update(bad)
        with pytest.raises(ValueError):
            au.write_song(tmp_path / "bad.midi", **args)
    (tmp_path / "cut.midi").write_bytes(open(tmp_path / "full.midi", "rb").read()[:-9])
    with pytest.raises(ValueError):
        au.read_song(tmp_path / "cut.midi")


# ------------------------------------------------------------------------------------------------------------------ the totals
def test_ratios_on_host_vectors():
    ratios = evaluation.InterplayTotals.ratios
    t = ir.Totals()
    assert len(t.vector()) == 166
    empty = ratios(t.vector())
    assert (empty["rows"], empty["songs"], empty["notes"], empty["pairs"], empty["ticks"]) == (0, 0, 0, 0, 0)
    assert all(math.isnan(empty[k]) for k in evaluation.InterplayTotals.RATIO_NAMES) and set(evaluation.InterplayTotals.RATIO_NAMES) < set(empty)
    # a melody (720) over a bass (723) and one row of a role outside 719..725
    out = dict(status=np.array([0, 0, 0, 1]), counts=np.array([[10, 0, 2, 8] + [0] * 4, [6, 1, 2, 6] + [0] * 4, [4, 0, 2, 1] + [0] * 4, [0] * 8]),
               pairs=np.array([[2, 1, 1, 0, 0, 4, 0, 1, 6], [1, 1, 0, 0, 0, 4, 0, 5, 1], [1, 0, 1, 0, 0, 0, 0, 1, 0], [0] * 9]),
               ticks=np.array([[200, 50, 50, 0, 0, 400, 0, 100, 600], [100, 50, 0, 0, 0, 400, 0, 450, 100], [100, 0, 50, 0, 0, 0, 0, 50, 0], [0] * 9]))
    meta = [META[:9] + [720] + META[10:], META[:9] + [723] + META[10:], META[:9] + [900] + META[10:], META]
    t.update(out, meta, songs=1)
    v = t.vector()
    assert v[:9] == [400, 100, 100, 0, 0, 800, 0, 600, 700] and v[18 + 9:18 + 18] == out["ticks"][0].tolist() and v[18 + 63:18 + 72] == out["ticks"][2].tolist()
    r = ratios(v)
    assert r == {"rows": 3, "songs": 1, "notes": 20, "pairs": 8, "ticks": 700, "dissonance": 200 / 1400, "unison": 400 / 1400,
                 "accompanied": 15 / 20, "bass_above": 100 / 550, "melody_below": 100 / 700}
    assert isinstance(r["rows"], int) and isinstance(r["unison"], float)
    text = evaluation.interplay_block(r)
    assert " Songs: 1 (3 tracks, 20 notes) " in text and " Dissonance: 0.142857 " in text and " Bass above: 0.181818 " in text and text.count("\n") == 10
    assert "nan" in evaluation.interplay_block(empty)


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    lib = _lib.lib()
    buf = (C.c_int64 * 64)()
    a = C.addressof(buf)
    ok = dict(notes=a, counts3=a, meta=a, valid=a, song=a, shift=a, counts=a, pairs=a, ticks=a, status=a, B=1, max_notes=4)
    bad = [dict(notes=None), dict(counts3=None), dict(meta=None), dict(counts=None), dict(pairs=None), dict(ticks=None), dict(status=None),
           dict(B=0), dict(B=-2), dict(max_notes=0), dict(max_notes=-1), dict(max_notes=32769), dict(B=65537, max_notes=32768),
           dict(B=2 ** 31 - 1, max_notes=2), dict(B=2 ** 30 + 1, max_notes=2)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mha_interplay_counts(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"interplay_counts" in lib.mh_last_error()
    assert not any(buf), "a refused call writes nothing"
    # the Python front refuses the same before it touches the library or asks for a device
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    for call in (lambda: metric.interplay_counts_raw(z(1, 4, 3), z(1, 3), z(1, 11)),
                 lambda: metric.interplay_counts_raw(z(1, 4), z(1, 3), z(1, 11)),
                 lambda: metric.interplay_counts_raw(z(1, 4, 4), z(1, 2), z(1, 11)),
                 lambda: metric.interplay_counts_raw(z(1, 4, 4), z(1, 3), z(2, 11)),
                 lambda: metric.interplay_counts_raw(z(1, 4, 4), z(1, 3), z(1, 11), song=z(2)),
                 lambda: metric.interplay_counts_raw(z(1, 4, 4), z(1, 3), z(1, 11), shift=z(1, 1)),
                 lambda: metric.interplay_counts_raw(z(1, 32769, 4), z(1, 3), z(1, 11)),
                 lambda: metric.interplay_counts_raw(z(0, 4, 4), z(0, 3), z(0, 11))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.MuseHipError):
        metric.interplay_counts_raw(z(1, 4, 4), z(1, 3), z(1, 11))                 # host tensors: there is no CPU path
