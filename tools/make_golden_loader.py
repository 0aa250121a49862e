#!/usr/bin/env python3
"""Generate tests/golden/loader.npz: what the REFERENCE's training-data path answers on seeded rows - data only.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_loader.py

Imports the reference read-only (MUSE_REFERENCE) behind the stand-ins tools/make_golden_encode.py and tools/make_golden_batch.py
already use (the `miditoolkit` and `datasets` stand-ins, the recording generator) and records four things:

 (a) merge, filter, collate   helper_tokenize and helper_filter (data/preprocess.py:26-81) on 40 synthetic (src, trg) rows with a seq_len
                              that leaves some out; collate_batches (data/wrapper.py:90-127) on index batches, bucketed and not
 (b) corruptions              Corruptions.__call__ per sequence (data/corruption.py:47-56) for "mt,mn,rn,rr" with corr_max 2 / 4 and
                              corr_p 0.5 / 1.0: the shuffled order, the slots that fired, the inner draws and the outputs
 (c) augmentation tables      for key_change -6..5 and both origins: the key number augment_by_key assigns (augment.py:40-59),
                              sync_key_augment (utils/utils.py:37-96) on every chord name of the vocabulary and its flat spellings,
                              encode_bpm (encoder/meta.py:119-123) over 5..220 combined with the five tempo changes
 (d) augmentation end to end  note lists through the reference's own augment_by_key / augment_by_bpm, Preprocessor._preprocess_midi_chunk
                              (preprocessor.py:190-275: sync_key_augment, MetaParser, MetaEncoder, EventSequenceEncoder) and
                              helper_tokenize, for several (key_change, bpm_change) each

What the stand-ins decide themselves, and the fixture says so (`d_standin_rules`): a MIDI file is a record in a dict here; its
dump() raises ValueError when a pitch leaves 0..127 - that rule is mido's (absent here), not something run from the reference; the
tempo PrettyMIDI reports is the record's tempo.  Everything else in (d) is the reference's code running.

The file is written with fixed zip timestamps, so a second run gives the same bytes."""
import contextlib
import io
import os
import random
import sys
import tempfile
import types
import zipfile
from pathlib import Path

import numpy as np
import torch

TOOLS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TOOLS)
sys.dont_write_bytecode = True
sys.path.insert(0, TOOLS)

import make_golden_encode as mge  # noqa: E402  (registers the stand-ins, puts the reference on sys.path)
import make_golden_batch as mgb  # noqa: E402  (Recorder)

from MuseDiffusion.data import corruption as rcorr  # noqa: E402
from MuseDiffusion.data.wrapper import collate_batches  # noqa: E402
from commu.preprocessor import augment as raug  # noqa: E402
from commu.preprocessor.encoder import EventSequenceEncoder, MetaEncoder  # noqa: E402
from commu.preprocessor.encoder.meta import encode_bpm  # noqa: E402
from commu.preprocessor.parser import MetaParser  # noqa: E402
from commu.preprocessor.preprocessor import Preprocessor  # noqa: E402
from commu.preprocessor.utils import sync_key_augment  # noqa: E402
from commu.preprocessor.utils.constants import KEY_MAP, KEY_NUM_MAP  # noqa: E402

rpre = mge.rpre


# ------------------------------------------------------------------------------------------------------------------ stand-ins
def _filter(self, fn, batched=True, num_proc=None, desc=None):
    """datasets.Dataset.filter, batched: keep the rows the function says True for"""
    keep = fn(dict(self.d))
    return mge.Dataset({k: [x for x, t in zip(v, keep) if t] for k, v in self.d.items()})


mge.Dataset.filter = _filter

FILES = {}   # path -> dict(tpb, notes [[start, end, pitch, velocity]], key, bpm): the "MIDI files" of part (d)


class KeySignature:
    def __init__(self, key_number):
        self.key_number = key_number


class MidiFile:
    """what augment.py, preprocessor.py and the encoder ask a miditoolkit.MidiFile for"""

    def __init__(self, path=None, *a, **k):
        f = FILES[str(path)]
        self.ticks_per_beat = f["tpb"]
        inst = mge.Instrument([mge.Note(int(v), int(p), int(s), int(e)) for s, e, p, v in f["notes"]])
        inst.name = "piano"
        self.instruments = [inst]
        self.key_signature_changes = [KeySignature(f["key"])]
        self.tempo_changes = [types.SimpleNamespace(tempo=f["bpm"], time=0)]

    def dump(self, path):
        notes = [[n.start, n.end, n.pitch, n.velocity] for n in self.instruments[0].notes]
        if any(not 0 <= n[2] <= 127 for n in notes):                  # the stand-in's own rule (mido: "data byte must be in range 0..127")
            raise ValueError("data byte must be in range 0..127")
        FILES[str(path)] = dict(tpb=self.ticks_per_beat, notes=notes, key=self.key_signature_changes[0].key_number,
                                bpm=self.tempo_changes[0].tempo)


class PrettyMIDI:
    def __init__(self, path):
        self.f = FILES[str(path)]

    def get_tempo_changes(self):
        return np.array([0.0]), np.array([float(self.f["bpm"])])

    def get_end_time(self):
        return 1.0


for _m in ("miditoolkit", "miditoolkit.midi.parser"):
    sys.modules[_m].MidiFile = MidiFile
sys.modules["miditoolkit"].TempoChange = lambda tempo, time: types.SimpleNamespace(tempo=tempo, time=time)
sys.modules["pretty_midi"].PrettyMIDI = PrettyMIDI

STANDIN_RULES = ("MidiFile.dump raises ValueError when a pitch leaves 0..127 (mido's rule, restated by the stand-in)",
                 "PrettyMIDI.get_tempo_changes reports the record's single tempo",
                 "sample_id_to_path lists the dumped records instead of walking a directory")


class Rec(mgb.Recorder):
    """+ the shuffled order, and marks around each corruption function's own draws"""

    def shuffle(self, x):
        self.r.shuffle(x)
        self.log.append(("order", [f.key for f in x]))


def ragged(lst, dtype=np.int32):
    return mge.ragged(lst, dtype)


# ------------------------------------------------------------------------------------------------------------------ (a) rows
ROOTS = ("A", "A#", "B", "C", "C#", "D", "D#", "E", "F", "F#", "G", "G#")
QUALS = ("", "7", "+", "dim", "m", "m7", "m7b5", "maj7", "sus4")


def make_rows(n=40, seed=11):
    """(src, trg): 11 meta tokens with an origin key for most rows; bars of notes with a chord event at the bar start"""
    g = random.Random(seed)
    src, trg = [], []
    for i in range(n):
        key = (602, 623)[i % 2] if i % 7 else g.randint(603, 625)
        src.append([g.randint(561, 600), key, g.randint(627, 629), g.randint(631, 637), g.randint(638, 640), g.randint(642, 649),
                    g.randint(651, 652), g.randint(654, 717), g.randint(654, 718), g.randint(720, 725), g.randint(727, 728)])
        t = []
        for _ in range(g.randint(2, 9)):
            t.append(2)
            t += [432, g.randint(195, 303)]
            for p in sorted(g.sample(range(432, 560), g.randint(1, 6))):
                if g.random() < 0.1:
                    t += [p, g.randint(195, 303)]
                else:
                    t += [p, g.randint(131, 194), g.randint(3 + 6, 130 - 6), g.randint(304, 431)]
        t.append(1)
        trg.append(t)
    return src, trg


def part_a(out):
    src, trg = make_rows()
    with contextlib.redirect_stdout(io.StringIO()):
        merged = rpre.helper_tokenize({"src": [list(s) for s in src], "trg": [list(t) for t in trg]}, num_proc=1)
    ids, mask, length = merged.d["input_ids"], merged.d["input_mask"], merged.d["length"]
    seq_len = sorted(length)[len(length) * 3 // 4]                       # a quarter of the rows is longer
    merged.d["row"] = list(range(len(ids)))                               # ours: which rows survive
    kept = rpre.helper_filter(merged, seq_len=seq_len, num_proc=1).d["row"]
    assert 0 < len(kept) < len(ids)
    out["a_src"], out["a_src_off"] = ragged(src)
    out["a_trg"], out["a_trg_off"] = ragged(trg)
    out["a_ids"], out["a_ids_off"] = ragged(ids)
    out["a_mask"], _ = ragged(mask)
    out["a_length"] = np.array(length, np.int32)
    out["a_seq_len"] = np.int32(seq_len)
    out["a_kept"] = np.array(kept, np.int32)
    # collate_batches on index batches over the FILTERED rows: sequential batches of 7 (what a deterministic DataLoader gives) and one
    # with repeated and descending indices
    nk = len(kept)
    batches = [list(range(lo, min(lo + 7, nk))) for lo in range(0, nk, 7)] + [[nk - 1, 3, 3, 0, nk - 2]]
    out["a_batches"], out["a_batches_off"] = ragged(batches)
    for j, idx in enumerate(batches):
        samples = [{"input_ids": torch.tensor(ids[kept[i]]), "input_mask": torch.tensor(mask[kept[i]]), "length": length[kept[i]]} for i in idx]
        for L, tag in ((None, "bucket"), (seq_len, "fixed")):
            for k, v in collate_batches(samples, seq_len=L).items():
                out["a_col%d_%s_%s" % (j, tag, k)] = v.numpy().astype(np.int32)
    return [ids[i] for i in kept], [mask[i] for i in kept]


# ------------------------------------------------------------------------------------------------------------------ (b) corruptions
AVAILABLE = ("mt", "mn", "rn", "rr")
CONFIGS = ((2, 0.5), (4, 0.5), (2, 1.0), (4, 1.0))


def part_b(out, rows, masks):
    rows = rows[:16]
    out["b_values"], out["b_off"] = ragged(rows)
    out["b_mask"], _ = ragged(masks[:16])
    out["b_available"] = np.array(AVAILABLE, dtype="U2")
    out["b_configs"] = np.array(CONFIGS, np.float64)
    off = out["b_off"]
    total = int(off[-1])
    rec_holder = {}

    def wrap(key):
        fn = rcorr.Corruptions.get(key)                                   # the reference's function with its default arguments bound

        def call(seq, inplace=False):
            rec_holder["rec"].log.append(("begin", key))
            res = fn(seq, inplace=inplace)
            rec_holder["rec"].log.append(("end", key))
            return res
        call.key = key
        return call

    for c, (corr_max, corr_p) in enumerate(CONFIGS):
        corr = rcorr.Corruptions(tuple(wrap(k) for k in AVAILABLE), corr_max, corr_p)
        choices = np.full((len(rows), corr_max), -1, np.int32)
        u = np.full((corr_max, total), 2.0, np.float64)                   # never < p
        new = np.zeros((corr_max, total, 3), np.int32)
        pairs = np.zeros((corr_max, len(rows), 3, 2), np.int32)
        pairs[..., 1] = 1
        outs = []
        for b, row in enumerate(rows):
            rec = rec_holder["rec"] = Rec(1000 * c + b)
            rcorr.generator = rec
            outs.append(corr(torch.tensor(row, dtype=torch.long)).numpy().astype(np.int32))
            log = rec.log
            assert log[0][0] == "order"
            order, at = log[0][1], 1
            for r in range(corr_max):
                assert log[at][0] == "u"
                fired = log[at][1] > 1 - corr_p
                at += 1
                if not fired:
                    continue
                key = order[r]
                assert log[at] == ("begin", key)
                end = log.index(("end", key), at)
                inner, at = log[at + 1:end], end + 1
                choices[b, r] = AVAILABLE.index(key)
                if key in ("mt", "mn"):
                    assert all(t == "u" for t, _ in inner)
                    u[r, off[b]:off[b] + len(inner)] = [v for _, v in inner]
                elif key == "rn":
                    k = j = 0
                    while j < len(inner):
                        assert inner[j][0] == "u"
                        u[r, off[b] + k] = inner[j][1]
                        if inner[j][1] < 0.5:
                            new[r, off[b] + k] = [inner[j + 1][1], inner[j + 2][1], inner[j + 3][1]]
                            j += 4
                        else:
                            j += 1
                        k += 1
                else:
                    assert len(inner) == 3 and all(t == "s" for t, _ in inner)
                    pairs[r, b] = [sorted(v) for _, v in inner]
            assert at == len(log)
        out["b%d_choices" % c] = choices
        out["b%d_u" % c], out["b%d_new" % c], out["b%d_pairs" % c] = u, new, pairs
        out["b%d_out" % c] = np.concatenate(outs)
        assert all(len(o) == len(r) for o, r in zip(outs, rows))
    # collate with correct_ids: the first config's outputs, bucketed and at a fixed width
    o0 = out["b0_out"]
    samples = [{"input_ids": torch.from_numpy(o0[off[b]:off[b + 1]].astype(np.int64)), "correct_ids": torch.tensor(rows[b]),
                "input_mask": torch.tensor(masks[b]), "length": len(rows[b])} for b in range(len(rows))]
    for L, tag in ((None, "bucket"), (max(len(r) for r in rows) + 3, "fixed")):
        for k, v in collate_batches(samples, seq_len=L).items():
            out["b_col_%s_%s" % (tag, k)] = v.numpy().astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ (c) tables
def part_c(out):
    keys = np.zeros((2, 12), np.int32)
    for o, origin in enumerate((0, 21)):
        for k in range(-6, 6):
            FILES["/c/key.mid"] = dict(tpb=480, notes=[[0, 10, 60, 64]], key=origin, bpm=120)
            with tempfile.TemporaryDirectory() as tmp:
                path = raug.augment_by_key("/c/key.mid", tmp, k)
            keys[o, k + 6] = FILES[path]["key"]
            assert Path(path).stem == "key_" + KEY_NUM_MAP[int(keys[o, k + 6])]
    out["c_key_numbers"] = keys                                           # [origin cmajor / aminor, key_change + 6]
    # sync_key_augment on every chord name of the vocabulary (capitalised, as the dataset writes them) and its flat spellings
    flats = {"A#": "Bb", "C#": "Db", "D#": "Eb", "F#": "Gb", "G#": "Ab"}
    names = [r + q for r in ROOTS for q in QUALS] + [flats[r] + q for r in ROOTS if r in flats for q in QUALS]
    table = np.zeros((2, 12, len(names)), dtype="U12")
    for o, origin in enumerate((0, 21)):
        for k in range(-6, 6):
            aug_key = KEY_NUM_MAP[int(keys[o, k + 6])].replace("minor", "").replace("major", "")   # preprocessor.py:238
            table[o, k + 6] = sync_key_augment(list(names), aug_key, KEY_NUM_MAP[origin][0])[0]
    out["c_chord_names"], out["c_chord_synced"] = np.array(names, dtype="U12"), table
    bpm = np.arange(5, 221)
    out["c_bpm"] = bpm.astype(np.int32)
    out["c_bpm_tokens"] = np.array([[encode_bpm(int(b) + 5 * c) for c in range(-2, 3)] for b in bpm], np.int32)   # [bpm, bpm_change + 2]


# ------------------------------------------------------------------------------------------------------------------ (d) end to end
T = 1920
PROGRESSIONS = (["C", "Am", "F", "G"], ["Am", "F", "C", "G7"], ["Dm7", "G7", "Cmaj7", "A7"], ["C", "C", "Fsus4", "G+"],
                ["Am", "Bm7b5", "E7", "Am"], ["F#dim", "G", "C#m", "D#7"], ["Bb", "Eb", "F", "Gm"], ["Csus2", "Am6", "Fadd2", "G7sus4"],
                ["Ab", "Dbmaj7", "Ebsus4", "Bbm7"], ["C6", "Ddim7", "Emadd2", "B"])   # no "NN": sync_key_augment's regex finds no root in it and the chunk dies on a TypeError
GRID = ((0, 0), (-6, -2), (-5, 2), (-3, 1), (-1, 0), (1, -1), (2, 2), (4, 0), (5, -2), (3, 2))


def make_cases(seed=5):
    """20 note lists: pitches kept 8 semitones inside 0..127 except the edge cases, which reach the ends on purpose"""
    g = np.random.default_rng(seed)
    cases = []
    for i in range(20):
        nm = (4, 8)[i % 2]
        n = int(g.integers(6, 40))
        lo, hi = (8, 120)
        if i == 17:
            lo, hi = 0, 40                                                # lowest pitch 0..: negative key changes leave the range
        if i == 18:
            lo, hi = 100, 128                                             # highest pitch ..127: positive ones do
        start = np.sort(g.integers(0, nm * T, n) // 60 * 60)
        notes = np.stack([start, start + g.integers(60, T, n), g.integers(lo, hi, n), g.integers(1, 128, n)], 1)
        if i == 17:
            notes[0, 2] = 3
        if i == 18:
            notes[0, 2] = 125
        prog = PROGRESSIONS[i % len(PROGRESSIONS)]
        names = [prog[(b * 2 + h) % 4] if i % 3 == 0 else prog[b % 4] for b in range(nm) for h in range(2) for _ in range(4)]
        key = ("cmajor", "aminor")[i % 2] if i != 19 else "dmajor"        # the last case: not an origin key
        meta = dict(bpm=(120, 60, 195, 10, 200, 95)[i % 6], audio_key=key, time_signature="4/4", pitch_range="mid", num_measures=nm,
                    inst=("acoustic_piano", "string_ensemble-2")[i % 2], genre=("newage", "cinematic")[i % 2], min_velocity=int(notes[:, 3].min()),
                    max_velocity=int(notes[:, 3].max()), track_role=("main_melody", "pad", "bass")[i % 3], rhythm="standard", sample_rhythm="standard")
        cases.append(("case%02d" % i, notes.astype(np.int64), names, meta))
    return cases


def part_d(out):
    cases = make_cases()
    pre = Preprocessor(meta_parser=MetaParser(), meta_encoder=MetaEncoder(), event_sequence_encoder=EventSequenceEncoder(), csv_path=None)
    rows = []          # (case, key_change, bpm_change, status, ids, mask)
    for ci, (name, notes, names, meta) in enumerate(cases):
        raw = "/raw/%s.mid" % name
        FILES[raw] = dict(tpb=480, notes=notes.tolist(), key=KEY_MAP[meta["audio_key"]], bpm=meta["bpm"])
        variants = {}                                                      # sample id -> (k, c)
        made = {name: raw}                                                 # _gather_sample_files: the raw directory first
        dropped = set()
        for k in sorted({k for k, _ in GRID}):
            with contextlib.redirect_stdout(io.StringIO()):
                tmp = raug.augment_by_key(raw, "/augmented_tmp", k)          # augment.py:35-70
            if tmp is None:
                dropped.add(k)
                continue
            for c in sorted({c for kk, c in GRID if kk == k}):
                before = set(FILES)
                raug.augment_by_bpm(tmp, "/augmented", c)                    # augment.py:73-85
                (path,) = set(FILES) - before
                variants[Path(path).stem] = (k, c)
                made[Path(path).stem] = path
        info = dict(meta, id=name, chord_progressions=[list(names)])
        with tempfile.TemporaryDirectory() as tmpdir, contextlib.redirect_stdout(io.StringIO()):
            pre._preprocess_midi_chunk((0, [info]), sample_id_to_path=dict(made), encode_tmp_dir=tmpdir)   # preprocessor.py:190-275
            got = {}
            for pos, sid in enumerate(made):
                p_in, p_tg = (os.path.join(tmpdir, "0000", "%s_%d.npy" % (kind, 1 + pos)) for kind in ("input", "target"))
                if sid in variants and os.path.exists(p_in):
                    got[variants[sid]] = ([int(t) for t in np.load(p_in, allow_pickle=True)], [int(t) for t in np.load(p_tg, allow_pickle=True)])
        for k, c in GRID:
            if (k, c) in got:
                src, trg = got[(k, c)]
                with contextlib.redirect_stdout(io.StringIO()):
                    d = rpre.helper_tokenize({"src": [src], "trg": [trg]}, num_proc=1).d
                rows.append((ci, k, c, 0, d["input_ids"][0], d["input_mask"][0]))
            else:
                status = 2 if k in dropped else 1                          # no variant: the file was dropped / the key is no origin
                assert status == 2 or meta["audio_key"] not in ("cmajor", "aminor")
                rows.append((ci, k, c, status, [], []))
    out["d_name"] = np.array([c[0] for c in cases], dtype="U8")
    out["d_notes"], out["d_notes_off"] = ragged([c[1] for c in cases])
    out["d_notes"] = out["d_notes"].reshape(-1, 4)
    out["d_notes_off"] //= 4
    out["d_chords"] = np.array([n for c in cases for n in c[2]], dtype="U12")
    out["d_chords_off"] = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])]).astype(np.int64)
    fields = ("bpm", "audio_key", "time_signature", "pitch_range", "num_measures", "inst", "genre", "min_velocity", "max_velocity",
              "track_role", "rhythm")
    out["d_meta_fields"] = np.array(fields, dtype="U16")
    out["d_meta_values"] = np.array([[str(c[3][f]) for f in fields] for c in cases], dtype="U24")
    out["d_case"] = np.array([r[0] for r in rows], np.int32)
    out["d_key_change"] = np.array([r[1] for r in rows], np.int32)
    out["d_bpm_change"] = np.array([r[2] for r in rows], np.int32)
    out["d_status"] = np.array([r[3] for r in rows], np.int32)            # 0 a variant exists, 1 not an origin key, 2 dropped for pitch range
    out["d_ids"], out["d_ids_off"] = ragged([r[4] for r in rows])
    out["d_mask"], _ = ragged([r[5] for r in rows])
    out["d_standin_rules"] = np.array(STANDIN_RULES, dtype="U128")
    # chord names in which the root string occurs twice (sync_key_augment:70 removes every occurrence): recorded as they are, listed here
    twice = sorted({n for c in cases for n in c[2] if n != "NN" and n.count(n[:2] if n[1:2] in ("#", "b") else n[:1]) > 1})
    out["d_root_twice"] = np.array(twice or [""], dtype="U12")
    return rows


def save(path, out):
    """np.savez_compressed with fixed zip timestamps (the same bytes on every run)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main():
    out = {}
    rows, masks = part_a(out)
    part_b(out, rows, masks)
    part_c(out)
    drows = part_d(out)
    path = os.path.join(REPO, "tests", "golden", "loader.npz")
    save(path, out)
    st = [r[3] for r in drows]
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays; (a)", len(out["a_length"]), "rows,", len(out["a_kept"]),
          "kept at seq_len", int(out["a_seq_len"]), "; (b)", [int((out["b%d_choices" % c] >= 0).sum()) for c in range(4)],
          "fired; (d)", len(drows), "rows: %d ok, %d not origin, %d pitch range" % (st.count(0), st.count(1), st.count(2)),
          "; root twice:", out["d_root_twice"].tolist())


if __name__ == "__main__":
    main()
