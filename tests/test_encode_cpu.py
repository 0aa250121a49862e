"""CPU: the numpy restatement of the encode path (tests/encode_ref.py) and the host half of utils/encode_util.py against what the
reference itself answered (tests/golden/encode.npz, tools/make_golden_encode.py), plus the MIDI reader against the MIDI writer.
The device kernels are compared with the same fixture in tests/test_encode_gpu.py."""
import ast
import os
import types

import numpy as np
import pytest
import torch

import encode_ref as er
from musediffusion_amd.utils import decode_util as mdec
from musediffusion_amd.utils import encode_util as menc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode.npz")
EXC_STATUS = {"": er.OK, "IndexError": er.EMPTY, "TypeError": er.NO_CHORDS, "ZeroDivisionError": er.BAD_TIMEBASE}
_CACHE = {}


def _cut(z, key, i):
    off = z[key + "_off"]
    return z[key][off[i]:off[i + 1]]


def fixture():
    if "z" not in _CACHE:
        _CACHE["z"] = dict(np.load(GOLDEN))
    return _CACHE["z"]


def fixture_cases():
    """-> list of namespaces: name, notes [k, 4], params (5,), names, words, oov, status (what the kernel must answer), ids, mask,
    length, clean.  Shared and never modified."""
    if "cases" not in _CACHE:
        z, out = fixture(), []
        for i, name in enumerate(z["name"]):
            status = EXC_STATUS[str(z["exc"][i]).split(":")[0]]
            if str(name).startswith("ours_"):                      # the reference encodes it; here it is BAD_CHORDS (documented)
                assert status == er.OK
                status = er.BAD_CHORDS
            num, den = (int(x) for x in z["ts"][i])
            params = np.array([z["tpb"][i], num, den, int(np.ceil(z["num_measures"][i])), z["inc"][i]], np.int32)
            out.append(types.SimpleNamespace(
                name=str(name), notes=_cut(z, "notes", i), params=params, names=[str(n) for n in _cut(z, "chord_names", i)],
                words=_cut(z, "words", i), oov=int(z["oov_lines"][i]), status=status, ids=_cut(z, "ids", i), mask=_cut(z, "mask", i),
                length=int(z["length"][i]), clean=bool(z["clean"][i])))
        _CACHE["cases"] = out
    return _CACHE["cases"]


def merge_cases():
    z = fixture()
    return [types.SimpleNamespace(name=str(n), trg=_cut(z, "merge_trg", i), ids=_cut(z, "merge_ids", i), mask=_cut(z, "merge_mask", i),
                                  length=int(z["merge_length"][i])) for i, n in enumerate(z["merge_name"])]


def meta_cases():
    z = fixture()
    fields = [str(f) for f in z["meta_fields"]]
    return [(str(n), {f: ast.literal_eval(str(v)) for f, v in zip(fields, z["meta_values"][i])}, _cut(z, "meta_tokens", i).tolist(),
             str(z["meta_exc"][i])) for i, n in enumerate(z["meta_name"])]


def test_fixture_covers_what_it_is_meant_to():
    cs = {c.name: c for c in fixture_cases()}
    assert len(cs) >= 60 and os.path.getsize(GOLDEN) < 128 * 1024
    assert {c.status for c in cs.values()} == {er.OK, er.EMPTY, er.NO_CHORDS, er.BAD_TIMEBASE, er.BAD_CHORDS}
    assert sorted(len(c.notes) for c in cs.values() if c.name.startswith("notes_") and c.name[6:].isdigit()) == [1, 255, 256, 257, 600]
    for ts in ("4_4", "3_4", "6_8", "12_8"):
        for tpb in (480, 96, 220):
            for inc in (0, 1):
                c = cs["sweep_%s_tpb%d_inc%d" % (ts, tpb, inc)]
                assert c.status == er.OK and c.params[3] == 17 and len(set(zip(c.names[:-1], c.names[1:]))) > 1
    assert sum(c.oov for c in cs.values()) > 20 and sum(c.clean for c in cs.values()) >= 30
    assert any(m.trg[0] >= 195 and m.trg[0] <= 303 for m in merge_cases())


def test_restatement_reproduces_every_fixture_case():
    for c in fixture_cases():
        words, counts, st = er.encode_events(c.notes, len(c.notes), c.params, er.chord_slots(c.names), len(c.names), er.MAX_ROW)
        assert st == c.status, (c.name, st, c.status)
        if c.status == er.OK:
            assert words == c.words.tolist(), c.name
            assert counts[1] == c.oov, (c.name, counts, c.oov)
            ids, mask = er.merge_row(fixture()["src"], words)
            assert ids == c.ids.tolist() and mask == c.mask.tolist() and len(ids) == c.length, c.name
        else:
            assert words == [] and counts == (0, 0), c.name
    for m in merge_cases():
        ids, mask = er.merge_row(fixture()["src"], m.trg)
        assert ids == m.ids.tolist() and mask == m.mask.tolist() and len(ids) == m.length, m.name


def test_restatement_overflow_and_hostile_counts():
    c = next(c for c in fixture_cases() if c.name == "simple")
    slots = er.chord_slots(c.names)
    assert er.encode_events(c.notes, len(c.notes), c.params, slots, len(slots), len(c.words))[2] == er.OK
    assert er.encode_events(c.notes, len(c.notes), c.params, slots, len(slots), len(c.words) - 1)[2] == er.OVERFLOW
    assert er.encode_events(c.notes, -3, c.params, slots, len(slots), 64)[2] == er.EMPTY
    assert er.encode_events(c.notes, len(c.notes) + 1, c.params, slots, len(slots), 64)[2] == er.OVERFLOW
    assert er.encode_events(c.notes, len(c.notes), c.params, slots, len(slots) + 1, 64)[2] == er.OVERFLOW
    assert er.encode_events(c.notes, len(c.notes), c.params, slots, -1, 64)[2] == er.NO_CHORDS


def test_host_chord_slots_match_the_restatement_and_the_vocabulary():
    """the host's table and the restatement's are two copies of one reading of the reference, so their equality only keeps them from
    drifting apart; what checks the string work is the fixture (chord names -> recorded words) and the hand-made names below"""
    assert menc.CHORD_VOCABULARY == er.CHORD_VOCABULARY and len(menc.CHORD_VOCABULARY) == 109 + 5 * 18 + 7 * 8
    assert menc.CHORD_NAMES == mdec.CHORD_NAMES
    for c in fixture_cases():
        assert np.array_equal(menc.chord_slots(c.names), er.chord_slots(c.names)), c.name
    s = menc.chord_slots(["C", "c", "C/E", "c/e", "Cmaj7(9)", "AbmM7", "Abm6", "Zz"])
    assert s[0, 0] == s[1, 0] != s[2, 0] == s[3, 0] and s[0, 1] == s[2, 1] == 195 + 27
    assert s[4, 1] == 195 + 27 + 7 and s[5, 1] == -1 and s[6, 1] == 195 + 99 + 4 and s[7, 1] == -1


def test_meta_to_sequence_reproduces_tokens_and_error_messages():
    m2s = menc.MetaToSequence()
    assert mdec.MetaToSequence is menc.MetaToSequence and issubclass(menc.UnprocessableMidiError, ValueError)
    seen = set()
    for name, meta, tokens, exc in meta_cases():
        kind, _, msg = exc.partition(": ")
        seen.add(kind)
        if not exc:
            assert m2s(dict(meta)) == tokens and m2s.execute(dict(meta)) == tokens, name
            assert m2s.encode_meta(meta) == tokens[:11] and m2s.encode_chord(meta["chord_progression"].split("-")) == tokens[11:], name
        elif kind == "UnprocessableMidiError":
            with pytest.raises(menc.UnprocessableMidiError) as e:
                m2s(dict(meta))
            assert str(e.value) == msg, name
        else:
            with pytest.raises({"KeyError": KeyError, "AssertionError": AssertionError}[kind]):
                m2s(dict(meta))
    assert seen == {"", "UnprocessableMidiError", "KeyError", "AssertionError"}
    with pytest.raises(menc.UnprocessableMidiError, match="Unprocessable midi"):
        m2s.encode_meta(dict(meta_cases()[0][1], num_measures="unknown"))


def test_read_midi_returns_what_write_midi_wrote(tmp_path):
    g = np.random.default_rng(3)
    start = np.sort(g.integers(0, 8000, 60))
    # distinct pitches but for the two pairs below: a file cannot say which of two overlapping notes of one pitch a note-off ends
    notes = np.stack([start, start + g.integers(1, 900, 60), g.permutation(128)[:60], g.integers(1, 128, 60)], 1).astype(np.int32)
    notes[5, :3] = notes[4, :3]                                     # the same pitch twice at one tick, equal ends
    notes[9, 0], notes[9, 2] = notes[8, 0], notes[8, 2]            # ... and with different ends: a note-off closes the oldest
    notes[9, 1] = notes[8, 1] + 17
    path = str(tmp_path / "a.mid")
    mdec.write_midi(path, notes, [(0, 200), (1920, 250)], [580, 610, 628])
    tpb, back = mdec.read_midi(path)
    assert tpb == mdec.TICKS_PER_BEAT and back.dtype == np.int32
    assert np.array_equal(back, notes)
    mdec.write_midi(path, notes[:0], [(0, 200)], [580, 610, 627])
    tpb, back = mdec.read_midi(path)
    assert tpb == 480 and back.shape == (0, 4)
    # format 0, 96 ticks, running status, note-on with velocity 0 as the note-off
    body = bytes([0, 0x90, 60, 100, 48, 64, 90, 48, 60, 0, 0, 0xFF, 0x06, 1, 65, 96, 64, 0, 0, 0xFF, 0x2F, 0])
    with open(path, "wb") as f:
        f.write(b"MThd" + (6).to_bytes(4, "big") + bytes([0, 0, 0, 1, 0, 96]) + b"MTrk" + len(body).to_bytes(4, "big") + body)
    tpb, back = mdec.read_midi(path)
    assert tpb == 96 and back.tolist() == [[0, 96, 60, 100], [48, 192, 64, 90]]
    with open(path, "wb") as f:
        f.write(b"RIFF....")
    with pytest.raises(ValueError):
        mdec.read_midi(path)
    # cut short anywhere, or an event that runs past its track chunk: ValueError, never IndexError
    head = b"MThd" + (6).to_bytes(4, "big") + bytes([0, 0, 0, 1, 0, 96]) + b"MTrk"
    whole = head + len(body).to_bytes(4, "big") + body
    for cut in range(1, len(whole)):
        with open(path, "wb") as f:
            f.write(whole[:cut])
        with pytest.raises(ValueError):
            mdec.read_midi(path)
    for short in (1, 2, 3, 5, 12, 13, len(body) - 2):                # the chunk says it is shorter than its events need
        with open(path, "wb") as f:
            f.write(head + short.to_bytes(4, "big") + body)
        try:
            mdec.read_midi(path)                                     # a chunk that happens to end between two events is a legal file
        except ValueError:
            pass
    with open(path, "wb") as f:
        f.write(head + (6).to_bytes(4, "big") + bytes([0, 0xFF, 0x06, 0x7F, 65, 66]))   # a text event of 127 bytes in a 6-byte chunk
    with pytest.raises(ValueError):
        mdec.read_midi(path)


class _Recorder:
    """stands in for the loaded library: records what mh_meta_to_batch is given, computes nothing"""

    def __init__(self):
        self.calls = []

    def mh_meta_to_batch(self, meta_ptr, n, ids, mask, B, L, stream):
        self.calls.append((meta_ptr, n, B, L))
        return 0


def test_meta_to_batch_takes_tokens_as_before_and_a_dict_through_meta_to_sequence(monkeypatch):
    rec, seen = _Recorder(), []
    monkeypatch.setattr(mdec, "lib", lambda: rec)
    monkeypatch.setattr(mdec, "current_stream", lambda: 0)
    monkeypatch.setattr(mdec, "ptr", lambda t: seen.append(t.clone()) or 0)
    name, meta, tokens, _ = meta_cases()[0]
    out = mdec.meta_to_batch(tokens, 3, 40, device="cpu")
    assert rec.calls[-1][1:] == (len(tokens), 3, 40) and seen[0].tolist() == tokens and seen[0].dtype == torch.int32
    assert set(out) == {"input_ids", "input_mask"} and out["input_ids"].shape == (3, 40) and out["input_mask"].dtype == torch.int32
    del seen[:]
    mdec.meta_to_batch(torch.tensor(tokens), 2, 32, device="cpu")
    assert rec.calls[-1][1:] == (len(tokens), 2, 32) and seen[0].tolist() == tokens
    del seen[:]
    mdec.meta_to_batch(dict(meta), 2, 32, device="cpu")
    assert rec.calls[-1][1:] == (len(tokens), 2, 32) and seen[0].tolist() == tokens
