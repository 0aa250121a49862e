"""CPU: the decode path's model and host half against the reference's recorded answers (tests/golden/decode.npz, made by
tools/make_golden_decode.py from the reference's own SequenceToMidi.decode with a recording stand-in for miditoolkit).

 - tests/decode_ref.py (the numpy restatement the GPU tests use at batch scale) reproduces every fixture case exactly;
 - the generated chord / key names and the tempo / time-signature formulas equal the recorded strings and numbers;
 - write_midi's files are read back by a minimal Standard MIDI File parser written here (byte equality with miditoolkit's dump
   cannot be checked: the package is not a dependency; the content is what is pinned);
 - the host half of decode_batch names and counts files as the reference does, in both modes."""
import os
import struct

import numpy as np
import pytest

import decode_ref as dr
from conftest import load_golden
from musediffusion_amd.utils import decode_util as mdec
from musediffusion_amd.utils.decode_util import (BAD_META, NO_EOS, OK, ONCE_FAILED, OVERFLOW, REF_INDEXERROR, RESTORE_FAILED, STRICT_FAILED,
                                                 DecodedRows, write_decoded_rows, write_midi)


def expected_status(exc):
    """the recorded exception of the reference -> status code"""
    if exc == "":
        return OK
    for text, st in (("NO EOS TOKEN", NO_EOS), ("RESTORE_CHORD FROM META FAILED", RESTORE_FAILED),
                     ("STRICT VALIDATION OF SEQUENCE FAILED", STRICT_FAILED), ("VALIDATION OF SEQUENCE FAILED", ONCE_FAILED)):
        if exc == "SequenceToMidiError: " + text:
            return st
    if exc.startswith("IndexError:"):
        return REF_INDEXERROR
    assert exc.startswith("KeyError:"), exc              # SIG_TIME_MAP / KEY_NUM_MAP lookups
    return BAD_META


class Case:
    def __init__(self, g, i):
        sl = lambda k: g[k][g[k + "_off"][i]:g[k + "_off"][i + 1]]
        self.name = str(g["name"][i])
        self.tokens, self.mask, self.restored, self.notes, self.marker_time = sl("tokens"), sl("mask"), sl("restored"), sl("notes"), sl("marker_time")
        self.marker_text = [str(t) for t in g["marker_text"][g["marker_time_off"][i]:g["marker_time_off"][i + 1]]]
        self.split_ok = str(g["split_exc"][i]) == ""
        self.split_status = expected_status(str(g["split_exc"][i]))
        self.status = {False: expected_status(str(g["exc"][i])), True: expected_status(str(g["exc_strict"][i]))}
        self.meta, self.tempo, self.ts, self.key_name = g["meta"][i], int(g["tempo"][i]), tuple(int(x) for x in g["ts"][i]), str(g["key_name"][i])
        self.oov, self.program, self.ticks_per_beat = int(g["oov_lines"][i]), int(g["program"][i]), int(g["ticks_per_beat"][i])


def fixture_cases():
    g = load_golden("decode.npz")
    return [Case(g, i) for i in range(len(g["name"]))]


def test_status_codes_mirror_the_header():
    assert (dr.OK, dr.NO_EOS, dr.RESTORE_FAILED, dr.ONCE_FAILED, dr.STRICT_FAILED, dr.REF_INDEXERROR, dr.BAD_META, dr.OVERFLOW) == \
        (OK, NO_EOS, RESTORE_FAILED, ONCE_FAILED, STRICT_FAILED, REF_INDEXERROR, BAD_META, OVERFLOW) == tuple(range(8))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "musehip.h")).read()
    for name, val in (("OK", OK), ("NO_EOS", NO_EOS), ("RESTORE_FAILED", RESTORE_FAILED), ("ONCE_FAILED", ONCE_FAILED),
                      ("STRICT_FAILED", STRICT_FAILED), ("REF_INDEXERROR", REF_INDEXERROR), ("BAD_META", BAD_META), ("OVERFLOW", OVERFLOW)):
        assert "MH_DECODE_%s = %d" % (name, val) in header
    assert sorted(mdec.STATUS_MESSAGE) == list(range(8))


def test_fixture_holds_the_cases_the_feature_is_pinned_by():
    cs = {c.name: c for c in fixture_cases()}
    st = [c.status[False] for c in cs.values()]
    for code in (OK, NO_EOS, RESTORE_FAILED, ONCE_FAILED, REF_INDEXERROR, BAD_META):
        assert code in st
    strict = [c.status[True] for c in cs.values()]
    assert STRICT_FAILED in strict and cs["strict_truncated_note"].status == {False: OK, True: REF_INDEXERROR}
    assert {c.ts for c in cs.values() if c.status[False] == OK} == {(4, 4), (3, 4), (6, 8), (12, 8)}
    assert len(cs["long_2096"].tokens) == 2096 and len(cs["long_300"].restored) > 256
    assert list(cs["eos_mid_truncated_note"].restored).index(1) < len(cs["eos_mid_truncated_note"].restored) - 1    # EOS not last
    assert list(cs["eos_twice"].restored).count(1) == 2
    assert any(c.oov for c in cs.values())


def test_restatement_reproduces_every_fixture_case():
    for c in fixture_cases():
        restored, meta, st, _ = dr.split_and_restore(c.tokens, c.mask, dr.MAX_ROW)
        assert st == c.split_status, c.name
        if c.split_ok:
            assert np.array_equal(restored, c.restored) and np.array_equal(meta, c.meta), c.name
        for strict in (False, True):
            r = dr.decode_row(c.tokens, c.mask, dr.MAX_ROW, 1024, 2048, strict)
            assert r["status"] == c.status[strict], (c.name, strict)
            if r["status"] == OK:
                assert np.array_equal(r["notes"], c.notes), c.name
                assert np.array_equal(r["chords"][:, 0], c.marker_time), c.name
                assert [mdec.CHORD_NAMES[t - 195] for t in r["chords"][:, 1]] == c.marker_text, c.name
                assert r["oov"] == c.oov and r["counts"] == (len(c.notes), len(c.marker_time), c.oov), c.name


def test_restatement_overflow_is_ours_and_only_a_matter_of_capacity():
    c = {c.name: c for c in fixture_cases()}["long_300"]
    n, k, m = len(c.restored), len(c.notes), len(c.marker_time)
    assert dr.decode_row(c.tokens, c.mask, n, k, m)["status"] == OK
    assert dr.decode_row(c.tokens, c.mask, n - 1, k, m)["status"] == OVERFLOW
    for cap in ((k - 1, m), (k, m - 1)):
        r = dr.decode_row(c.tokens, c.mask, n, *cap)
        assert r["status"] == OVERFLOW and r["counts"] == (k, m, 0) and len(r["notes"]) == 0
    assert dr.decode_row(c.tokens, np.full_like(c.mask, 7), n, k, m)["status"] == BAD_META      # sum(mask) > L
    assert dr.decode_row(c.tokens, -np.ones_like(c.mask), n, k, m)["status"] == BAD_META        # sum(mask) < 0


def test_names_and_meta_formulas_equal_the_recorded_ones():
    assert len(mdec.CHORD_NAMES) == 109 and len(set(mdec.CHORD_NAMES)) == 109 and len(set(mdec.KEY_NAMES)) == 24
    keys, chords = set(), set()
    for c in fixture_cases():
        if c.status[False] != OK:
            continue
        assert mdec.KEY_NAMES[c.meta[1] - 602] == c.key_name and (c.meta[0] - 560) * 5 == c.tempo, c.name
        assert mdec.TIME_SIGNATURES[c.meta[2] - 627] == c.ts and c.ticks_per_beat == mdec.TICKS_PER_BEAT and c.program == 0, c.name
        keys.add(c.key_name)
        chords.update(c.marker_text)
    assert keys == set(mdec.KEY_NAMES) and chords == set(mdec.CHORD_NAMES)     # every generated name is pinned by a recorded one


# ---------------------------------------------------------------------------------------------- a minimal Standard MIDI File parser
def _read_vlq(buf, i):
    v = 0
    while True:
        v = (v << 7) | (buf[i] & 0x7F)
        i += 1
        if not buf[i - 1] & 0x80:
            return v, i


def parse_midi(path):
    """-> dict(format, division, tracks = list of lists of (tick, kind, payload)): meta events ('meta', type, bytes), channel
    events ('on' / 'off' / 'program', channel, data...).  No running status, no sysex: the writer uses neither."""
    buf = open(path, "rb").read()
    assert buf[:4] == b"MThd"
    hlen, fmt, ntrk, div = struct.unpack(">IHHH", buf[4:14])
    assert hlen == 6
    i, tracks = 14, []
    for _ in range(ntrk):
        assert buf[i:i + 4] == b"MTrk"
        (tlen,) = struct.unpack(">I", buf[i + 4:i + 8])
        i += 8
        end, tick, ev = i + tlen, 0, []
        while i < end:
            d, i = _read_vlq(buf, i)
            tick += d
            s = buf[i]
            if s == 0xFF:
                n, j = _read_vlq(buf, i + 2)
                ev.append((tick, "meta", buf[i + 1], bytes(buf[j:j + n])))
                i = j + n
            elif s & 0xF0 in (0x80, 0x90):
                ev.append((tick, "on" if s & 0xF0 == 0x90 else "off", s & 0x0F, buf[i + 1], buf[i + 2]))
                i += 3
            else:
                assert s & 0xF0 == 0xC0, hex(s)
                ev.append((tick, "program", s & 0x0F, buf[i + 1]))
                i += 2
        assert i == end and ev[-1][1:3] == ("meta", 0x2F), "track must end with end-of-track, exactly at its length"
        tracks.append(ev)
    assert i == len(buf)
    return dict(format=fmt, division=div, tracks=tracks)


def check_midi_file(path, notes, chords, meta):
    """the file holds exactly this music: header, tempo, both signatures, markers, program, every note's on / off"""
    m = parse_midi(path)
    assert (m["format"], m["division"], len(m["tracks"])) == (1, 480, 2)
    t0, t1 = m["tracks"]
    metas = {e[2]: e for e in t0 if e[2] in (0x51, 0x58, 0x59)}
    assert all(e[0] == 0 for e in metas.values()) and len(metas) == 3
    bpm = (int(meta[0]) - 560) * 5
    assert int.from_bytes(metas[0x51][3], "big") == round(60_000_000 / bpm)
    num, den = mdec.TIME_SIGNATURES[int(meta[2]) - 627]
    assert metas[0x58][3][0] == num and 2 ** metas[0x58][3][1] == den
    sf, mi = struct.unpack(">bB", metas[0x59][3])
    name = mdec.KEY_NAMES[int(meta[1]) - 602]
    # circle of fifths, written out independently of the writer's table: major keys by number of sharps (+) / flats (-)
    major_by_sf = {0: "c", 1: "g", 2: "d", 3: "a", 4: "e", 5: "b", -1: "f", -2: "bb", -3: "eb", -4: "ab", -5: "db", -6: "gb"}
    minor_by_sf = {0: "a", 1: "e", 2: "b", 3: "gb", 4: "db", 5: "ab", -1: "d", -2: "g", -3: "c", -4: "f", -5: "bb", -6: "eb"}   # sharp minors under the flat names the key table uses
    assert name == (minor_by_sf if mi else major_by_sf)[sf] + ("minor" if mi else "major")
    markers = [(e[0], e[3].decode()) for e in t0 if e[2] == 0x06]
    assert markers == sorted(((int(t), mdec.CHORD_NAMES[int(c) - 195]) for t, c in chords), key=lambda x: x[0])
    assert t1[0] == (0, "program", 0, 0)
    ons = sorted((e[0], e[3], e[4]) for e in t1 if e[1] == "on")
    offs = sorted((e[0], e[3]) for e in t1 if e[1] == "off")
    assert all(e[2] == 0 for e in t1 if e[1] in ("on", "off"))
    assert ons == sorted((int(s), int(p), int(v)) for s, _, p, v in notes)
    assert offs == sorted((int(e), int(p)) for _, e, p, _ in notes)
    ticks = [e[0] for e in t1]
    assert ticks == sorted(ticks)


def test_write_midi_round_trip(tmp_path):
    n = 0
    for c in fixture_cases():
        if c.status[False] != OK or not (c.name.startswith(("key_", "sweep_", "long_300", "change_two")) or c.name == "eos_twice"):
            continue
        r = dr.decode_row(c.tokens, c.mask, dr.MAX_ROW, 1024, 2048)
        path = str(tmp_path / (c.name + ".midi"))
        write_midi(path, r["notes"], r["chords"], r["meta"])
        check_midi_file(path, c.notes, list(zip(c.marker_time, r["chords"][:, 1])), c.meta)
        n += 1
    assert n >= 30
    with pytest.raises(ValueError):
        write_midi(str(tmp_path / "x.midi"), np.zeros((0, 4)), np.zeros((0, 2)), [560, 602, 627])      # tempo 0


def rows_from_restatement(tokens, masks, strict=False):
    rs = dr.decode_rows(tokens, masks, 2 * tokens.shape[1], tokens.shape[1] // 2, tokens.shape[1], strict)
    return rs, DecodedRows(np.array([r["status"] for r in rs], np.int32), np.stack([r["meta"] for r in rs]),
                           np.array([r["counts"] for r in rs], np.int32), [r["notes"] for r in rs], [r["chords"] for r in rs])


def test_decode_batch_file_names_and_counts_in_both_modes(tmp_path, capsys):
    keep = [k for k in dr.BATCH_KINDS if k not in ("no_chords", "bad_meta")][::3]
    tokens, masks, _ = dr.make_batch(3, 320, keep)
    for strict in (False, True):
        rs, rows = rows_from_restatement(tokens, masks, strict)
        bad = [i for i, r in enumerate(rs) if r["status"] != OK]
        assert all(rs[i]["status"] in (NO_EOS, RESTORE_FAILED, ONCE_FAILED, STRICT_FAILED) for i in bad) and 4 <= len(bad) < len(rs) - 4
        gen, mod = tmp_path / ("gen%d" % strict), tmp_path / ("mod%d" % strict)
        gen.mkdir(), mod.mkdir()
        assert write_decoded_rows("generation", rows, 2, 40, str(gen), return_indices=True) == (len(rs) - len(bad), bad)
        assert write_decoded_rows("generation", rows, 2, 40, str(gen)) == len(rs) - len(bad)
        assert sorted(os.listdir(gen)) == ["generated_%07d.midi" % (40 + k) for k in range(len(rs) - len(bad))]      # valid rows numbered densely
        assert write_decoded_rows("modification", rows, 7, 100, str(mod), return_indices=True) == (len(rs) - len(bad), bad)
        good = [i for i in range(len(rs)) if i not in bad]
        assert sorted(os.listdir(mod)) == ["%07d_batch%05d_%04d.midi" % (100 + i, 7, i) for i in good]                # named by original index
        for k, i in enumerate(good[:6]):
            for path in (gen / ("generated_%07d.midi" % (40 + k)), mod / ("%07d_batch%05d_%04d.midi" % (100 + i, 7, i))):
                check_midi_file(str(path), rs[i]["notes"], rs[i]["chords"], rs[i]["meta"])
    out = capsys.readouterr().out
    assert "Summary of Trial 2" in out and "Summary of Batch 7" in out and "Generation Failure: NO EOS TOKEN" in out and "OOV:" in out


def test_decode_batch_raises_where_the_reference_would(tmp_path):
    for kind, exc in (("no_chords", IndexError), ("bad_meta", KeyError)):
        tokens, masks, _ = dr.make_batch(4, 320, ("clean", kind, "clean"))
        _, rows = rows_from_restatement(tokens, masks)
        for mode in ("generation", "modification"):
            with pytest.raises(exc):
                write_decoded_rows(mode, rows, 0, 0, str(tmp_path))
    with pytest.raises(AssertionError):
        write_decoded_rows("other", rows, 0, 0, str(tmp_path))
