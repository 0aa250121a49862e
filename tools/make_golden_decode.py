#!/usr/bin/env python3
"""Generate tests/golden/decode.npz: what the REFERENCE's token -> MIDI decode path answers on hand-made and seeded rows.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_decode.py

Imports the reference read-only (MUSE_REFERENCE, as tools/make_golden_batch.py does) and runs its own
SequenceToMidi.split_meta_midi and SequenceToMidi.decode (utils/decode_util.py:192-211, through commu's
EventSequenceEncoder.decode / encoder_utils.write_midi).  `miditoolkit` is absent; write_midi uses it only as a container
for its result, so a recording stand-in made here is registered under that name: plain classes that keep what they are given.

Per case the fixture holds data only: the row and its mask, split_meta_midi's two outputs (or the exception's name), and
for strict_validation False and True either the decoded notes / markers / tempo / time signature / key name / number of
"OOV" lines printed, or the exception's class name and message.  Ragged fields are stored flat with an offsets array."""
import contextlib
import io
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MUSE_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


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
    def __init__(self, program, is_drum=False, name=""):
        self.program, self.is_drum, self.name, self.notes = program, is_drum, name, []


class TimeSignature:
    def __init__(self, numerator, denominator, time):
        self.numerator, self.denominator, self.time = numerator, denominator, time


class KeySignature:
    def __init__(self, key_name, time):
        self.key_name, self.time = key_name, time


class TempoChange:
    def __init__(self, tempo, time):
        self.tempo, self.time = tempo, time


class Marker:
    def __init__(self, text, time):
        self.text, self.time = text, time


class MidiFile:
    def __init__(self, *a, **k):
        self.ticks_per_beat = None
        self.time_signature_changes, self.key_signature_changes, self.tempo_changes = [], [], []
        self.instruments, self.markers = [], []


def _register():
    for name in ("logger", "parmap", "pretty_midi"):
        sys.modules.setdefault(name, _Stub(name))
    top, midi, parser, cont = (_Stub("miditoolkit"), _Stub("miditoolkit.midi"), _Stub("miditoolkit.midi.parser"),
                               _Stub("miditoolkit.midi.containers"))
    for cls in (Note, Instrument, TimeSignature, KeySignature, TempoChange, Marker):
        setattr(top, cls.__name__, cls)
        setattr(cont, cls.__name__, cls)
    top.MidiFile = parser.MidiFile = MidiFile
    top.midi, midi.parser, midi.containers = midi, parser, cont
    for m in (top, midi, parser, cont):
        sys.modules[m.__name__] = m


_register()
from MuseDiffusion.utils import decode_util as rdec  # noqa: E402
import decode_ref as dr  # noqa: E402  (only its row generator: the fixture's answers all come from the reference)

META = [580, 610, 627, 633, 639, 644, 651, 660, 700, 720, 727]


def row(meta, chord, notes, L=None, sep=(0,), mask_shift=0):
    pre = list(meta) + list(chord)
    r = pre + list(sep) + list(notes)
    L = len(r) + 3 if L is None else L
    assert len(r) <= L
    n0 = len(pre) + len(sep) + mask_shift
    return np.array(r + [0] * (L - len(r)), np.int64), np.array([0] * n0 + [1] * (L - n0), np.int64)


def N(pos, vel=150, pitch=60, dur=320):
    return [432 + pos, vel, pitch, dur]


def with_ts(ts):
    m = list(META)
    m[2] = ts
    return m


def cases():
    c = []
    def add(name, r):
        assert len(r[0]) == len(r[1]), name
        c.append((name, r[0], r[1]))

    two_bars = [2] + N(0) + N(40, 140, 64) + N(100, 160, 67) + [2] + N(10, 131, 3, 304) + N(90, 194, 130, 431)
    # --- the three entry branches of restore_chord
    add("branch_equal", row(META, [432, 200, 432, 210], two_bars + [1]))
    add("branch_one_more", row(META, [432, 200, 432, 210], [2] + two_bars + [1]))
    add("branch_fewer", row(META, [432, 200, 432, 210, 432, 220, 432, 230], two_bars + [1]))
    add("branch_fewer_by_one_no_bar", row(META, [432, 200], N(5) + N(9) + [1]))
    # --- chord changes inside a bar: with a candidate note, without one, two in one bar, at the very last position
    add("change_with_candidate", row(META, [432, 200, 496, 205, 432, 210, 480, 215], two_bars + [1]))
    add("change_without_candidate", row(META, [432, 200, 432, 210, 440, 215], two_bars + [1]))
    add("change_two_in_bar", row(META, [432, 200, 464, 201, 528, 202, 432, 210, 448, 211, 544, 212], two_bars + [1]))
    add("change_candidate_is_chord_free_bar", row(META, [432, 200, 448, 201, 432, 210], [2, 2] + N(3) + [1]))
    add("change_decreasing_positions", row(META, [432, 200, 544, 201, 464, 202, 432, 210], two_bars + [1]))   # last_idx moves backwards
    add("change_unsorted_notes", row(META, [432, 200, 480, 201, 432, 210], [2] + N(100) + N(20) + N(110) + [2] + N(1) + [1]))
    # --- an EOS that lands mid-sequence: the candidate sits in the last three tokens, the slice runs over the end
    add("eos_mid_truncated_note", row(META, [432, 200, 544, 201], [2] + N(0) + [432 + 50, 150, 1]))
    add("eos_mid_position_only", row(META, [432, 200, 432, 210, 544, 211], two_bars + [432 + 99, 1]))
    add("eos_twice", row(META, [432, 200, 560, 201, 464, 202], [2] + N(8) + N(70) + [432 + 80, 1]))
    # --- the event pass: the last three events are not matched; OOV tokens dropped before matching
    add("trailing_chord_dropped", row(META, [432, 200, 432, 210, 496, 215], [2] + N(0) + [2] + N(3) + [1]))
    add("trailing_bar", row(META, [432, 200, 432, 210], [2] + N(0) + N(9) + [2, 1]))
    add("oov_inside_note", row(META, [432, 200, 432, 210], [2, 432, 0, 150, 600, 60, 728, 320] + N(7) + [2] + N(1) + [0, 0, 1]))
    add("oov_after_eos_cut", row(META, [432, 200], [2] + N(0) + N(4) + [1, 500, 150, 60, 320, 1, 2]))
    add("one_note_only", row(META, [432, 200], [2] + N(0) + [1]))
    add("first_token_is_a_note", row(META, [432, 200, 432, 210], N(0) + [2] + N(4) + [2] + N(8) + [1]))
    # --- every position, velocity, pitch and duration under each time signature (4/4, 3/4, 6/8, 12/8)
    for ts in (627, 628, 629, 630):
        sweep = [2]
        for k in range(128):
            sweep += [432 + k, 131 + k % 64, 3 + k, 304 + (127 - k if k % 2 else k)]
        sweep += [2] + N(127, 194, 127, 431) + N(1) + [2] + N(64) + [1]
        add("sweep_ts_%d" % ts, row(with_ts(ts), [432, 200, 480, 250, 432, 303, 432, 195, 496, 260], sweep))
    # --- every key name and every chord name: 24 keys, five chords each over 195..303
    for k in range(24):
        m = list(META)
        m[1], m[0] = 602 + k, 561 + (k * 7) % 40
        chord, notes = [], []
        for j in range(5):
            chord += [432, 195 + (5 * k + j) % 109]
            notes += [2] + N(3 * j + k, 131 + k, 40 + j, 304 + 5 * j)
        add("key_%d" % (602 + k), row(m, chord, notes + [1]))
    # --- failures
    add("no_eos", row(META, [432, 200], [2] + N(0) + N(4)))
    add("no_eos_notes_empty", row(META, [432, 200], []))
    add("too_many_bars", row(META, [432, 200, 432, 210], [2, 2] + two_bars + [1]))
    add("empty_chords_no_bar", row(META, [], N(0) + N(4) + [1]))
    add("empty_chords_one_bar", row(META, [], [2] + N(0) + N(4) + [1]))
    add("empty_chords_two_bars", row(META, [], two_bars + [1]))
    add("just_eos", row(META, [432, 200, 432, 210], [1]))
    add("just_eos_empty_chords", row(META, [], [1]))
    add("chords_only_notes", row(META, [432, 200, 432, 210], [2, 2, 1]))
    add("strict_truncated_note", row(META, [432, 200, 432, 210], two_bars + [432 + 120, 150, 1]))
    add("strict_truncated_position", row(META, [432, 200, 432, 210], two_bars + [432 + 120, 1]))
    add("strict_bad_order", row(META, [432, 200, 432, 210], [2] + N(0) + [150, 60] + [2] + N(3) + [1]))
    add("bad_time_signature_low", row(with_ts(626), [432, 200], [2] + N(0) + N(4) + [1]))
    add("bad_time_signature_high", row(with_ts(631), [432, 200], [2] + N(0) + N(4) + [1]))
    m = list(META); m[1] = 601
    add("bad_key_low", row(m, [432, 200], [2] + N(0) + N(4) + [1]))
    m = list(META); m[1] = 626
    add("bad_key_high", row(m, [432, 200], [2] + N(0) + N(4) + [1]))
    # --- hostile but legal: chord parts no encoder writes, masks that split elsewhere
    add("chord_part_odd_length", row(META, [432, 200, 432], two_bars + [1]))
    add("chord_part_432_at_odd_index", row(META, [432, 432, 432, 210], [2] + two_bars + [2] + N(3) + [1]))
    add("chord_part_starts_with_change", row(META, [448, 200, 432, 210], [2] + N(0) + N(4) + [1]))
    add("chord_part_runs_out_of_bars", row(META, [200, 432, 432, 210, 432, 220], two_bars + [1]))
    add("chord_value_huge", row(META, [432, 200, 728, 0], two_bars + [1]))
    add("mask_all_ones", (np.array([2] + N(0) + N(5) + N(9) + N(12) + [1], np.int64), np.ones(18, np.int64)))
    add("mask_one_zero", (np.array([2] + N(0) + N(5) + N(9) + N(12) + [1], np.int64), np.array([0] + [1] * 17, np.int64)))
    add("mask_all_zero", (np.array(META + [432, 200, 0, 2] + N(0) + [1], np.int64), np.zeros(20, np.int64)))
    add("mask_one_short", row(META, [432, 200, 432, 210], two_bars + [1], mask_shift=-1))
    add("mask_one_long", row(META, [432, 200, 432, 210], two_bars + [1], mask_shift=1))
    add("meta_five_tokens", (np.array(META[:5] + [0, 2] + N(0) + N(3) + [2] + N(5) + [2, 1], np.int64),
                             np.array([0] * 6 + [1] * 16, np.int64)))
    # --- long rows: more than 256 note tokens, and the reference's longest seq_len
    g = np.random.default_rng(11)
    meta, chord = dr.make_meta(g, 6, 2, ts=627)
    add("long_300", row(meta, chord, dr.make_notes(g, 6, 12), L=400))
    meta, chord = dr.make_meta(g, 16, 3, ts=628)
    add("long_2096", row(meta, chord, [2] + dr.make_notes(g, 16, 30), L=2096))
    # --- seeded rows of every perturbation kind the generator knows
    for kind in dr.KINDS:
        for k in range(2):
            t, m = dr.make_row(g, 320, kind)
            add("gen_%s_%d" % (kind, k), (t.astype(np.int64), m.astype(np.int64)))
    return c


def exc_name(e):
    return "%s: %s" % (type(e).__name__, e)


def main():
    S = rdec.SequenceToMidi
    flat = {k: [] for k in ("tokens", "mask", "restored", "notes", "marker_time", "marker_text")}
    rec = {k: [] for k in ("name", "split_exc", "meta", "exc", "exc_strict", "tempo", "ts", "key_name", "oov_lines", "program", "ticks_per_beat")}
    for name, seq, mask in cases():
        flat["tokens"].append(seq.astype(np.int32))
        flat["mask"].append(mask.astype(np.int32))
        rec["name"].append(name)
        try:
            note_seq, meta = S.split_meta_midi(seq.copy(), mask.copy())
            rec["split_exc"].append("")
            flat["restored"].append(np.asarray(note_seq, np.int32))
            m11 = np.zeros(11, np.int32)
            m11[:len(meta)] = meta
            rec["meta"].append(m11)
        except Exception as e:  # noqa: BLE001 - the class name is the datum
            rec["split_exc"].append(exc_name(e))
            flat["restored"].append(np.zeros(0, np.int32))
            rec["meta"].append(np.zeros(11, np.int32))
        results = []
        for strict in (False, True):
            out = io.StringIO()
            try:
                with contextlib.redirect_stdout(out):
                    midi = S(strict_validation=strict).decode(seq.copy(), mask.copy())
                results.append(("", midi, out.getvalue()))
            except Exception as e:  # noqa: BLE001
                results.append((exc_name(e), None, out.getvalue()))
        rec["exc"].append(results[0][0])
        rec["exc_strict"].append(results[1][0])
        midi, log = results[0][1], results[0][2]
        if midi is None:
            flat["notes"].append(np.zeros((0, 4), np.int32))
            flat["marker_time"].append(np.zeros(0, np.int32))
            flat["marker_text"].append([])
            for k, v in (("tempo", 0), ("ts", (0, 0)), ("key_name", ""), ("oov_lines", 0), ("program", -1), ("ticks_per_beat", 0)):
                rec[k].append(v)
        else:
            assert len(midi.instruments) == 1 and len(midi.tempo_changes) == 1 and midi.tempo_changes[0].time == 0
            inst = midi.instruments[0]
            flat["notes"].append(np.array([[n.start, n.end, n.pitch, n.velocity] for n in inst.notes], np.int32).reshape(-1, 4))
            flat["marker_time"].append(np.array([mk.time for mk in midi.markers], np.int32))
            flat["marker_text"].append([str(mk.text) for mk in midi.markers])
            ts, ks = midi.time_signature_changes[0], midi.key_signature_changes[0]
            assert ts.time == 0 and ks.time == 0 and not inst.is_drum
            rec["tempo"].append(int(midi.tempo_changes[0].tempo))
            rec["ts"].append((ts.numerator, ts.denominator))
            rec["key_name"].append(str(ks.key_name))
            rec["oov_lines"].append(sum(1 for ln in log.splitlines() if ln.startswith("OOV")))
            rec["program"].append(int(inst.program))
            rec["ticks_per_beat"].append(int(midi.ticks_per_beat))
            if results[1][1] is not None:                   # strict validation only rejects: same music when it passes
                a, b = results[0][1].instruments[0].notes, results[1][1].instruments[0].notes
                assert [(n.start, n.end, n.pitch, n.velocity) for n in a] == [(n.start, n.end, n.pitch, n.velocity) for n in b]
    out = {}
    for k in ("tokens", "mask", "restored", "marker_time"):
        out[k] = np.concatenate(flat[k]).astype(np.int32)
        out[k + "_off"] = np.concatenate([[0], np.cumsum([len(a) for a in flat[k]])]).astype(np.int64)
    out["notes"] = np.concatenate(flat["notes"]).astype(np.int32)
    out["notes_off"] = np.concatenate([[0], np.cumsum([len(a) for a in flat["notes"]])]).astype(np.int64)
    out["marker_text"] = np.array([t for lst in flat["marker_text"] for t in lst] or [""], dtype="U16")
    for k in ("name", "split_exc", "exc", "exc_strict", "key_name"):
        out[k] = np.array(rec[k], dtype="U96")
    out["meta"] = np.stack(rec["meta"])
    for k in ("tempo", "oov_lines", "program", "ticks_per_beat"):
        out[k] = np.array(rec[k], np.int32)
    out["ts"] = np.array(rec["ts"], np.int32)
    path = os.path.join(REPO, "tests", "golden", "decode.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(rec["name"]), "cases")
    for i, nm in enumerate(rec["name"]):
        print("%-36s split=%-40s exc=%-50s strict=%s notes=%d markers=%d oov=%d" % (
            nm, rec["split_exc"][i][:40], rec["exc"][i][:50], rec["exc_strict"][i][:50], len(flat["notes"][i]),
            len(flat["marker_time"][i]), rec["oov_lines"][i]))


if __name__ == "__main__":
    main()
