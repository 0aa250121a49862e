#!/usr/bin/env python3
"""Generate tests/golden/encode.npz: what the REFERENCE's notes -> tokens encode path answers on hand-made and seeded rows.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_encode.py

Imports the reference read-only (MUSE_REFERENCE, as tools/make_golden_decode.py does) and runs its own
EventSequenceEncoder.encode (commu/preprocessor/encoder/encoder.py:21-69), MetaToSequence (utils/decode_util.py:16-50) and
helper_tokenize's merge_and_mask (data/preprocess.py:26-70).  `miditoolkit` and `datasets` are absent; the encoder uses the
first only to get a note list and a tick base, the tokenizer the second only for from_dict + map, so stand-ins made here are
registered under those names: a MidiFile that hands back the note list registered under the "path" it is given, and a Dataset
that applies the mapped function to its dict.

Per case the fixture holds data only: the inputs (notes, time base, chord names), the words or the exception's class name,
the number of "OOV" lines printed, the reference's merged ids / mask / length for the fixed 11-token meta below, and a flag set
here: whether the reference's own split_meta_midi applied to its own merged row returns the words again.  Merge-only cases
(hand-made word rows) and MetaToSequence cases (dict -> tokens or the exception's message) follow.  Ragged fields are stored
flat with an offsets array."""
import contextlib
import importlib.util
import io
import math
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MUSE_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        m = _Stub(self.__name__ + "." + k)
        setattr(self, k, m)
        return m

    def __call__(self, *a, **k):
        return self


class Note:
    def __init__(self, velocity, pitch, start, end):
        self.velocity, self.pitch, self.start, self.end = velocity, pitch, start, end


class Instrument:
    def __init__(self, notes):
        self.notes = notes


FILES = {}   # "path" -> (ticks_per_beat, [[start, end, pitch, velocity], ...])


class MidiFile:
    """the two things the encoder asks a MidiFile for: ticks_per_beat and instruments[0].notes (fresh objects per open)"""

    def __init__(self, path=None, *a, **k):
        tpb, notes = FILES[path]
        self.ticks_per_beat = tpb
        self.instruments = [Instrument([Note(int(v), int(p), int(s), int(e)) for s, e, p, v in notes])]


class Dataset:
    def __init__(self, d):
        self.d = d

    @classmethod
    def from_dict(cls, d):
        return cls(dict(d))

    def map(self, fn, batched=True, num_proc=None, remove_columns=(), desc=None):
        out = fn(dict(self.d))
        return Dataset({k: v for k, v in out.items() if k not in remove_columns})


def _register():
    for name in ("logger", "parmap", "pretty_midi"):
        sys.modules.setdefault(name, _Stub(name))
    top, midi, parser, cont = (_Stub("miditoolkit"), _Stub("miditoolkit.midi"), _Stub("miditoolkit.midi.parser"),
                               _Stub("miditoolkit.midi.containers"))
    top.MidiFile = parser.MidiFile = MidiFile
    top.midi, midi.parser, midi.containers = midi, parser, cont
    for m in (top, midi, parser, cont):
        sys.modules[m.__name__] = m
    ds = types.ModuleType("datasets")
    ds.Dataset = Dataset
    sys.modules["datasets"] = ds


_register()
from MuseDiffusion.utils import decode_util as rdec  # noqa: E402
from commu.preprocessor.encoder import EventSequenceEncoder  # noqa: E402

_spec = importlib.util.spec_from_file_location("_ref_preprocess", os.path.join(REF, "MuseDiffusion", "data", "preprocess.py"))
rpre = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rpre)

META = [580, 610, 627, 633, 639, 644, 651, 660, 700, 720, 727]
BEATS = {"4/4": 4, "3/4": 3, "6/8": 3, "12/8": 6}


def N(start, dur=100, pitch=60, vel=80):
    return [start, start + dur, pitch, vel]


def bars_of(names, cpb):
    """one name per bar -> a progression with no change inside a bar"""
    return [n for n in names for _ in range(cpb)]


def cases():
    """-> list of (name, notes, ticks_per_beat, time signature, num_measures, is_incomplete_measure, chord names)"""
    c = []

    def add(name, notes, tpb=480, ts="4/4", nm=4, inc=0, chords=None):
        cpb = 2 * BEATS[ts]
        chords = bars_of(["C", "Am", "F", "G"], cpb) if chords is None else chords
        c.append((name, np.array(notes, np.int64).reshape(-1, 4), tpb, ts, nm, inc, list(chords)))

    T = 1920
    simple = [N(0), N(480, 240, 64), N(960, 480, 67), N(T + 120, 60, 62), N(2 * T + 1000, 900, 72, 100), N(3 * T + 1900, 10, 50, 30)]
    add("simple", simple)
    add("simple_reversed_input", simple[::-1])
    # --- order: (start, pitch, input order)
    add("equal_start_unequal_pitch", [N(480, 100, 70), N(480, 200, 60), N(480, 300, 65), N(0, 50, 90), N(3 * T, 100)])
    add("equal_start_equal_pitch", [N(480, 100, 60, 10), N(480, 900, 60, 120), N(480, 300, 60, 64), N(3 * T, 100)])
    add("equal_start_last_sorted_decides_max_time", [N(0), N(T, 3 * T, 80), N(T, 10, 90)])       # the last sorted note ends in bar 1
    # --- group_items: downbeats from the LAST sorted note's end
    add("last_note_ends_early", [N(0, 4 * T), N(T + 5), N(2 * T + 5), N(2 * T + 100, 10)])
    add("last_note_end_before_start", [N(0), N(T + 5), [3 * T, 2 * T - 1, 60, 80]])             # the bar of the last note is lost
    add("last_note_end_before_start_far", [N(0), N(T + 5), [3 * T, 1, 60, 80]])                 # downbeats [0, T): only bar 0
    add("last_note_end_negative", [N(0), [T, -T - 1, 60, 80]])                                    # no downbeat pair: chords only
    add("last_note_end_on_downbeat", [N(0), N(T - 100, 100)])                                     # arange stops before max_time + T
    add("negative_start", [[-10, 50, 60, 80], [-1, 5, 61, 80], N(0), N(T)])
    add("empty_bars_between", [N(0), N(3 * T + 7)])
    add("notes_on_bar_boundaries", [N(0), N(T - 1, 10), N(T, 10), N(2 * T - 8, 10), N(2 * T - 7, 10), N(3 * T, 10), N(4 * T - 1, 10)])
    # --- position: first argmin, ties (ticks_per_bar 256 and 768: flags 2 and 6 ticks apart)
    add("position_ties_tpb64", [N(s, 20) for s in (0, 1, 2, 3, 5, 253, 254, 255, 256, 257, 511)], tpb=64)
    add("position_ties_tpb192", [N(s, 20) for s in (0, 2, 3, 4, 9, 15, 21, 764, 765, 766, 767, 768, 771)], tpb=192)
    add("position_last_flag", [N(T - 15, 5), N(T - 8, 5), N(T - 7, 5), N(T - 1, 5), N(2 * T - 1, 5)])
    # --- velocity / pitch / duration bins
    add("velocity_edges", [N(100 * k, 50, 60, v) for k, v in enumerate((0, 1, 2, 3, 4, 5, 63, 64, 65, 125, 126, 127, 128, 200, -3))])
    add("pitch_edges", [N(100 * k, 50, p) for k, p in enumerate((-1, 0, 1, 127, 128, 300))])
    add("duration_edges", [N(100 * k, d) for k, d in enumerate((-50, 0, 1, 7, 8, 15, 22, 23, 1912, 1913, 1920, 1927, 1928, 5000))])
    add("duration_oov_tpb220", [N(100 * k, d) for k, d in enumerate((1, 6, 9, 765, 768, 771, 774, 876, 880, 2000))], tpb=220)
    add("all_oov_note", [[0, 10, -1, 0], N(T)])
    # --- chord side
    cp = bars_of(["C", "Am", "F", "G"], 8)
    add("chords_change_inside_bars", simple, chords=["C", "C", "C", "C", "Am", "Am", "Am", "Am"] + ["F"] * 7 + ["G"] + ["C", "D", "E", "F", "G", "A", "B", "C"] + ["C"] * 8)
    add("chords_same_across_bars", simple, chords=["C"] * 32)
    add("chords_case_and_slash", simple, chords=["C", "c", "C/E", "c/e", "C/G", "C", "Cmaj7(9)", "Cmaj7"] + ["Am/C"] * 8 + ["F(add9)"] * 8 + ["G7/B"] * 8)
    add("chords_flat_and_abstract", simple, chords=["Ab", "Bbm7", "Dbmaj7", "Ebsus2", "Gb7sus4", "Abdim7", "Bb6", "Ebm6"] +
        ["Csus2", "Dadd2", "E6", "Fdim7", "G7sus4", "Am6", "Bmadd2", "CmM7"] + ["Abmaj", "Dbadd2", "EbmM7", "Gbmadd2", "Bb+", "Abm7b5", "Dbsus4", "Ebm"] +
        ["C#m6", "F#6", "Cmaj", "NN", "nn", "H7", "", "X"])
    add("chords_unknown_every_bar", simple, chords=bars_of(["Zz", "Q7", "C9", "Cb"], 8))
    add("num_measures_short", simple, nm=2)
    add("num_measures_long", simple, nm=7)
    add("num_measures_zero", simple, nm=0)
    add("num_measures_float", simple, nm=3.5)
    add("incomplete_first_measure", [N(T - 200, 100), N(T), N(2 * T + 100), N(4 * T + 50)], nm=5, inc=1, chords=cp)
    add("incomplete_changes_inside", [N(T - 200, 100), N(T + 240), N(2 * T + 100), N(4 * T + 50)], nm=4.5, inc=1,
        chords=["C", "D", "D", "E", "E", "E", "F", "G"] * 4)
    add("incomplete_short_measures", [N(100), N(T + 240)], nm=2, inc=1, chords=cp)
    add("incomplete_as_bool", [N(100), N(T + 240)], nm=5, inc=True, chords=cp)
    add("note_and_chord_same_time", [N(0), N(240), N(T), N(T + 960), N(3 * T)], chords=["C", "D"] * 16)
    # --- every slot a change, 17 measures, each time signature at each tick base
    for ts in ("4/4", "3/4", "6/8", "12/8"):
        for tpb in (480, 96, 220):
            cpb = 2 * BEATS[ts]
            tbar = int(tpb * (int(ts.split("/")[0]) / int(ts.split("/")[1]) * 4))
            names = [("C", "Dm", "Eb7", "F#dim", "Gsus4")[k % 5] for k in range(17 * cpb)]
            g = np.random.default_rng(tpb + cpb)
            notes = [N(int(s), int(d), int(p), int(v)) for s, d, p, v in zip(g.integers(0, 17 * tbar, 40), g.integers(1, tbar, 40),
                                                                             g.integers(30, 100, 40), g.integers(1, 128, 40))]
            for inc in (0, 1):
                add("sweep_%s_tpb%d_inc%d" % (ts.replace("/", "_"), tpb, inc), notes, tpb=tpb, ts=ts, nm=17, inc=inc, chords=names)
    # --- failures
    add("no_notes", [])
    add("no_chords", simple, chords=[])
    add("bad_timebase_tpb16", simple, tpb=16)                                                     # ticks_per_bar 64: step 0
    add("bad_timebase_tpb31", simple, tpb=31)                                                     # 124
    add("timebase_tpb32", [N(0, 5), N(100, 3), N(130, 300)], tpb=32)                              # 128: the smallest that works
    add("ours_uneven_chords", simple, chords=cp[:-3])                                             # array_split splits unevenly: BAD_CHORDS here
    # --- sizes: one, around the block size, and more than one item per thread
    g = np.random.default_rng(7)
    for n in (1, 255, 256, 257, 600):
        s = g.integers(0, 16 * T, n)
        s = (s // 60) * 60 if n != 257 else s
        notes = np.stack([s, s + g.integers(1, T, n), g.integers(0, 128, n), g.integers(0, 130, n)], 1)
        add("notes_%d" % n, notes, nm=16, chords=bars_of(["C", "Am", "F", "G"] * 4, 8))
    return c


def merge_cases():
    """hand-made word rows for merge_and_mask alone: what the encoder cannot be made to write"""
    return [("merge_no_chord", [2, 432, 150, 60, 320, 1]),
            ("merge_chord_at_index_0", [200, 432, 150, 60, 320, 1]),                              # the pair is (-1, 0): -1 is the last element
            ("merge_adjacent_chords", [2, 432, 200, 201, 440, 150, 60, 320, 1]),
            ("merge_three_adjacent", [2, 432, 200, 201, 202, 1]),
            ("merge_chords_only", [195, 303, 250]),
            ("merge_chord_last", [2, 432, 150, 60, 320, 1, 303]),
            ("merge_chord_first_and_last", [195, 2, 432, 150, 60, 320, 303]),
            ("merge_single_chord", [250]),
            ("merge_single_eos", [1]),
            ("merge_bounds", [194, 195, 303, 304, 1])]


def meta_cases():
    base = dict(bpm=120, audio_key="aminor", time_signature="4/4", pitch_range="mid_high", num_measures=8.0, inst="acoustic_piano",
                genre="newage", min_velocity=60, max_velocity=80, track_role="main_melody", rhythm="standard",
                chord_progression="Am-Am-Am-Am-Am-Am-Am-Am-G-G-G-G-G-G-G-G-F-F-F-F-F-F-F-F-E-E-E-E-E-E-E-E")
    c = [("meta_base", base)]

    def var(name, **kw):
        c.append((name, dict(base, **kw)))

    var("meta_bpm_low", bpm=3)
    var("meta_bpm_high", bpm=400)
    var("meta_bpm_7", bpm=7)
    var("meta_keys", audio_key="c#major")
    var("meta_key_flat", audio_key="bbminor")
    var("meta_key_unknown", audio_key="unknown")
    var("meta_key_bad", audio_key="hmajor")
    var("meta_ts_12_8", time_signature="12/8")
    var("meta_ts_unknown", time_signature="unknown")
    var("meta_ts_bad", time_signature="5/4")
    var("meta_pitch_range_bad", pitch_range="middle")
    var("meta_pitch_range_unknown", pitch_range="unknown")
    for nm in (4, 5, 8.5, 9, 16, 17, 17.9, 7, 18, 0):
        var("meta_measures_%s" % str(nm).replace(".", "_"), num_measures=nm)
    var("meta_inst_vocal", inst="vocal")
    var("meta_inst_bad", inst="kazoo")
    var("meta_inst_unknown", inst="unknown")
    var("meta_genre_cinematic", genre="cinematic")
    var("meta_genre_bad", genre="jazz")
    var("meta_genre_unknown", genre="unknown")
    var("meta_velocity_odd", min_velocity=61, max_velocity=127)
    var("meta_velocity_zero", min_velocity=0, max_velocity=1)
    var("meta_track_role_riff", track_role="riff")
    var("meta_track_role_bad", track_role="solo")
    var("meta_track_role_unknown", track_role="unknown")
    var("meta_rhythm_triplet", rhythm="triplet")
    var("meta_rhythm_bad", rhythm="swing")
    var("meta_rhythm_unknown", rhythm="unknown")
    var("meta_chord_changes", chord_progression="C-C-D-D-E-F-G-A-A#m7-A#m7-A#m7-A#m7-Bsus4-Bsus4-Bsus4-C")
    var("meta_chord_unknown", chord_progression="C-C-C-C-H-H-H-H")
    var("meta_chord_lowercase", chord_progression="c-c-c-c-c-c-c-c")
    var("meta_chord_uneven", chord_progression="C-C-C-C-C-C-C")
    return c


def exc_name(e):
    return "%s: %s" % (type(e).__name__, e)


def ragged(lst, dtype=np.int32):
    lst = [np.asarray(a, dtype).reshape(-1) for a in lst]
    return (np.concatenate(lst).astype(dtype) if lst else np.zeros(0, dtype),
            np.concatenate([[0], np.cumsum([len(a) for a in lst])]).astype(np.int64))


def merge_ref(trg):
    """helper_tokenize (through the datasets stand-in) on one (META, trg) pair -> (ids, mask, length, round trip flag)"""
    with contextlib.redirect_stdout(io.StringIO()):
        d = rpre.helper_tokenize({"src": [list(META)], "trg": [list(trg)]}, num_proc=1).d
    ids, mask, length = d["input_ids"][0], d["input_mask"][0], d["length"][0]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            back, meta = rdec.SequenceToMidi.split_meta_midi(np.array(ids, np.int64), np.array(mask, np.int64))
        clean = list(np.asarray(back).tolist()) == [int(t) for t in trg] and list(np.asarray(meta).tolist())[:11] == META
    except Exception:  # noqa: BLE001 - a row the reference cannot split again is simply not clean
        clean = False
    return ids, mask, length, clean


def main():
    enc = EventSequenceEncoder()
    rec = {k: [] for k in ("name", "exc", "tpb", "ts", "num_measures", "inc", "oov_lines", "length", "clean")}
    flat = {k: [] for k in ("notes", "words", "ids", "mask")}
    chords = []
    for name, notes, tpb, ts, nm, inc, names in cases():
        FILES[name] = (tpb, notes.tolist())
        info = {"chord_progressions": [names], "num_measures": nm, "time_signature": ts, "is_incomplete_measure": inc}
        out = io.StringIO()
        try:
            with contextlib.redirect_stdout(out):
                words = [int(w) for w in enc.encode(name, sample_info=info)]
            exc = ""
        except Exception as e:  # noqa: BLE001 - the class name is the datum
            words, exc = [], exc_name(e)
        rec["name"].append(name)
        rec["exc"].append(exc)
        rec["tpb"].append(tpb)
        rec["ts"].append([int(x) for x in ts.split("/")])
        rec["num_measures"].append(float(nm))
        rec["inc"].append(int(inc))
        rec["oov_lines"].append(sum(1 for ln in out.getvalue().splitlines() if ln.startswith("OOV")))
        flat["notes"].append(notes)
        flat["words"].append(words)
        chords.append(names)
        if exc:
            ids, mask, length, clean = [], [], 0, False
        else:
            ids, mask, length, clean = merge_ref(words)
        flat["ids"].append(ids)
        flat["mask"].append(mask)
        rec["length"].append(length)
        rec["clean"].append(clean)
    out = {}
    for k in ("notes", "words", "ids", "mask"):
        out[k], out[k + "_off"] = ragged(flat[k])
    out["notes"] = out["notes"].reshape(-1, 4)
    out["notes_off"] //= 4
    out["chord_names"] = np.array([n for names in chords for n in names] or [""], dtype="U16")
    out["chord_names_off"] = np.concatenate([[0], np.cumsum([len(n) for n in chords])]).astype(np.int64)
    out["name"] = np.array(rec["name"], dtype="U48")
    out["exc"] = np.array(rec["exc"], dtype="U96")
    for k in ("tpb", "inc", "oov_lines", "length"):
        out[k] = np.array(rec[k], np.int32)
    out["ts"] = np.array(rec["ts"], np.int32)
    out["num_measures"] = np.array(rec["num_measures"], np.float64)
    out["clean"] = np.array(rec["clean"], np.bool_)
    out["src"] = np.array(META, np.int32)
    # merge-only cases
    mrec = [(name, trg) + merge_ref(trg) for name, trg in merge_cases()]
    out["merge_name"] = np.array([m[0] for m in mrec], dtype="U48")
    out["merge_trg"], out["merge_trg_off"] = ragged([m[1] for m in mrec])
    out["merge_ids"], out["merge_ids_off"] = ragged([m[2] for m in mrec])
    out["merge_mask"], out["merge_mask_off"] = ragged([m[3] for m in mrec])
    out["merge_length"] = np.array([m[4] for m in mrec], np.int32)
    out["merge_clean"] = np.array([m[5] for m in mrec], np.bool_)
    # MetaToSequence cases: the dict as parallel arrays of field values (strings), the tokens or the exception
    m2s = rdec.MetaToSequence()
    mc = meta_cases()
    fields = list(mc[0][1].keys())
    out["meta_name"] = np.array([n for n, _ in mc], dtype="U48")
    out["meta_fields"] = np.array(fields, dtype="U24")
    out["meta_values"] = np.array([[repr(d[f]) for f in fields] for _, d in mc], dtype="U128")
    toks, excs = [], []
    for _, d in mc:
        try:
            toks.append([int(t) for t in m2s(dict(d))])
            excs.append("")
        except BaseException as e:  # noqa: BLE001 - AssertionError included
            toks.append([])
            excs.append(exc_name(e))
    out["meta_tokens"], out["meta_tokens_off"] = ragged(toks)
    out["meta_exc"] = np.array(excs, dtype="U160")
    path = os.path.join(REPO, "tests", "golden", "encode.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(rec["name"]), "cases")
    for i, nm in enumerate(rec["name"]):
        print("%-44s exc=%-40s notes=%3d words=%4d oov=%2d merged=%4d clean=%d" % (
            nm, rec["exc"][i][:40], len(flat["notes"][i]), len(flat["words"][i]), rec["oov_lines"][i], rec["length"][i], rec["clean"][i]))
    for m in mrec:
        print("%-44s length=%d clean=%d ids=%s" % (m[0], m[4], m[5], m[2]))
    for (n, _), t, e in zip(mc, toks, excs):
        print("%-44s %s" % (n, e[:100] if e else t))


def time_reference(rows=32):
    """--time-reference: the reference's own encode + merge_and_mask on the first `rows` of tests/encode_ref.bench_items(), one core"""
    import time
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import encode_ref as er
    items = er.bench_items()
    enc = EventSequenceEncoder()
    infos = []
    for k, it in enumerate(items[:rows]):
        tpb, num, den, nm, inc = (int(x) for x in it["params"])
        FILES[k] = (tpb, it["notes"].tolist())
        infos.append({"chord_progressions": [it["names"]], "num_measures": nm, "time_signature": "%d/%d" % (num, den), "is_incomplete_measure": inc})
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        words = [enc.encode(k, sample_info=info) for k, info in enumerate(infos)]
    t1 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        rpre.helper_tokenize({"src": [list(META)] * rows, "trg": [w.tolist() for w in words]}, num_proc=1)
    t2 = time.perf_counter()
    for w, it in zip(words, items):
        assert w.tolist() == er.encode_events(it["notes"], len(it["notes"]), it["params"], er.chord_slots(it["names"]), len(it["names"]), 4096)[0]
    print("reference, one CPU core, %d of %d rows (%d notes): encode %.1f ms per row, merge_and_mask %.2f ms per row -> %.0f ms + %.0f ms per %d-row batch"
          % (rows, len(items), sum(len(it["notes"]) for it in items[:rows]), (t1 - t0) / rows * 1e3, (t2 - t1) / rows * 1e3,
             (t1 - t0) / rows * len(items) * 1e3, (t2 - t1) / rows * len(items) * 1e3, len(items)))


if __name__ == "__main__":
    time_reference() if "--time-reference" in sys.argv[1:] else main()
