"""Grammar-constrained rounding without a device: the restatement tests/grammar_ref.py against brute-force enumeration of every accepted
string, constrained rows through the decode restatement (tests/decode_ref.py, strict), every status on hand-made rows, the refusals."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as dr
import grammar_ref as gr
from musediffusion_amd import _lib


def int_tables(g, n, lo=-64, hi=64):
    """integer scores (exact in fp32, sums too) and distinct indices per slot"""
    cs = g.integers(lo, hi + 1, (n, 8)).astype(np.float32)
    ci = np.tile(np.arange(8, dtype=np.int32) * 10, (n, 1)) + g.integers(0, 10, (n, 8)).astype(np.int32)
    return cs, ci


# ------------------------------------------------------------------------------------------------------------------ brute force
def test_restatement_equals_brute_force_on_tiny_rows():
    g = np.random.default_rng(1)
    tied = no_room = checked = 0
    for case in range(400):
        n = int(g.integers(5, 13))
        hi = int(g.integers(0, 3))
        lo = int(g.integers(0, hi + 1))
        cs, ci = int_tables(g, n)
        st, classes, total, counts = gr.viterbi(cs, ci, lo, hi)
        best, score = gr.brute_force(cs, lo, hi)
        if not best:
            assert st == gr.NO_ROOM and n < lo + 5, (case, n, lo, hi)
            no_room += 1
            continue
        assert st == gr.OK and float(total) == score, (case, st, total, score)
        if len(best) > 1:
            tied += 1
            assert tuple(classes) in best, case
            continue
        assert tuple(classes) == best[0], (case, classes, best[0])
        s = list(classes)
        assert counts == (s.count(gr.BAR), s.count(gr.DURATION), s.index(gr.EOS) + 1) and lo <= counts[0] <= hi
        checked += 1
    print("brute force: %d checked, %d tied, %d without room" % (checked, tied, no_room))
    assert tied <= 20 and no_room > 0 and checked > 300


def test_accepted_strings_are_the_grammar():
    """the enumeration itself: every string parses under the header's automaton and none is listed twice"""
    for n, lo, hi in ((5, 0, 0), (6, 0, 1), (9, 0, 2), (10, 1, 1), (12, 2, 2), (12, 0, 2)):
        strings = gr.accepted_strings(n, lo, hi)
        assert len({tuple(s) for s in strings}) == len(strings) > 0
        for s in strings:
            assert len(s) == n
            e = s.index(gr.EOS)
            assert all(c == gr.PAD for c in s[e + 1:])
            body, i, notes = s[:e], 0, 0
            while i < len(body):
                if body[i] == gr.BAR:
                    i += 1
                else:
                    assert body[i:i + 4] == [gr.POSITION, gr.VELOCITY, gr.PITCH, gr.DURATION], s
                    i, notes = i + 4, notes + 1
            assert notes >= 1 and lo <= body.count(gr.BAR) <= hi
    assert gr.accepted_strings(4, 0, 2) == [] and gr.accepted_strings(6, 2, 2) == []
    assert gr.accepted_strings(5, 0, 0) == [[gr.POSITION, gr.VELOCITY, gr.PITCH, gr.DURATION, gr.EOS]]


# ------------------------------------------------------------------------------------------------------------------ through the decoder
def random_row_tables(g, ids, mask, pad_bias):
    """class scores [L, 8] and indices for one row: slots 0..6 a random token of the class, slot 7 the best of them inside the note
    region and the row's own token in front of it (the anchored prefix)"""
    L = len(ids)
    cs = g.standard_normal((L, 8)).astype(np.float32) * np.float32(2)
    cs[:, gr.PAD] += np.float32(pad_bias)
    ci = np.zeros((L, 8), np.int32)
    for c, (lo, hi) in enumerate(gr.NOTE_CLASSES):
        ci[:, c] = g.integers(lo, hi, L)
    top = cs[:, :7].argmax(1)
    cs[:, 7] = cs[np.arange(L), top]
    ci[:, 7] = ci[np.arange(L), top]
    len_meta = L - int(mask.sum())
    ci[:len_meta, 7] = ids[:len_meta]
    return cs, ci


def test_constrained_rows_decode_strictly_and_the_plain_argmax_does_not():
    g = np.random.default_rng(5)
    L = 160
    ok = {gr.BARS_EXACT: 0, gr.BARS_DECODABLE: 0}
    plain_ok = 0
    bars_seen = set()
    for case in range(96):
        n_bars = 1 + case % 8
        ids, mask = dr.make_row(g, L, "clean", n_bars=n_bars, notes_per_bar=2)
        cs, ci = random_row_tables(g, ids, mask, pad_bias=(0.0, 1.5, 4.0)[case % 3])
        len_meta = L - int(mask.sum())
        plain = dr.decode_row(ci[:, 7], mask, 2 * L, L, L, strict=True)
        plain_ok += plain["status"] == dr.OK
        for policy in (gr.BARS_EXACT, gr.BARS_DECODABLE):
            r = gr.constrain_row(cs, ci, ids, mask, policy)
            assert r["status"] == gr.OK, (case, policy, r["status"])
            tok = r["tokens"]
            assert np.array_equal(tok[:len_meta], ids[:len_meta])
            d = dr.decode_row(tok, mask, 2 * L, L, L, strict=True)
            assert d["status"] == dr.OK, (case, policy, d["status"])
            bars, notes, through = r["counts"]
            region = list(tok[len_meta:])
            assert region.count(dr.BAR) == bars and region.index(dr.EOS) + 1 == through and all(t == 0 for t in region[through:])
            assert d["counts"][0] == notes >= 1
            if policy == gr.BARS_EXACT:
                assert bars == n_bars
            else:
                assert 0 <= bars <= n_bars + 1
                # the wider policy can only score higher
                assert r["path_score"] >= gr.constrain_row(cs, ci, ids, mask, gr.BARS_EXACT)["path_score"]
                bars_seen.add(bars - n_bars)
            ok[policy] += 1
    assert ok == {gr.BARS_EXACT: 96, gr.BARS_DECODABLE: 96}
    assert plain_ok == 0                                            # random tokens per position: the decoder rejects every such row
    assert len(bars_seen) > 1


# ------------------------------------------------------------------------------------------------------------------ statuses
def hand_row(g, L=64, n_bars=2):
    ids, mask = dr.make_row(g, L, "clean", n_bars=n_bars, notes_per_bar=1)
    cs, ci = random_row_tables(g, ids, mask, 0.0)
    return ids, mask, cs, ci


def test_every_status_on_hand_made_rows():
    g = np.random.default_rng(11)
    ids, mask, cs, ci = hand_row(g)
    L = len(ids)
    len_meta = L - int(mask.sum())
    run = lambda **kw: gr.constrain_row(kw.pop("cs", cs), kw.pop("ci", ci), kw.pop("ids", ids), kw.pop("mask", mask), **kw)  # noqa: E731
    assert run()["status"] == gr.OK and run()["counts"][0] == 2
    plain = ci[:, 7]
    # a mask that leaves no region, and one that is no 0 / 1 mask
    for m in (np.zeros(L, np.int32), np.full(L, 2, np.int32), -np.ones(L, np.int32)):
        r = run(mask=m)
        assert r["status"] == gr.BAD_MASK and np.array_equal(r["tokens"], plain) and r["counts"] == (0, 0, 0) and r["path_score"] == 0
    r = run(mask=np.ones(L, np.int32))                              # len_meta 0: the whole row is the region, ids[11:-1] the chord part
    assert r["status"] == gr.OK and r["counts"][0] == list(ids[11:-1]).count(432) == list(r["tokens"]).count(2)
    no_chords = ids.copy()
    no_chords[11:len_meta - 1][no_chords[11:len_meta - 1] == 432] = 433
    for policy in (gr.BARS_EXACT, gr.BARS_DECODABLE):
        assert run(ids=no_chords, policy=policy)["status"] == gr.NO_CHORDS
    assert run(ids=no_chords, lo=0, hi=3)["status"] == gr.OK       # explicit bounds do not ask the meta
    assert run(lo=0, hi=64)["status"] == gr.TOO_MANY_BARS and run(lo=0, hi=63)["status"] == gr.OK
    assert run(lo=-1, hi=3)["status"] == gr.BAD_BOUNDS and run(lo=3, hi=2)["status"] == gr.BAD_BOUNDS
    assert run(lo=-1, hi=64)["status"] == gr.TOO_MANY_BARS          # the order of the header
    n = L - len_meta
    assert run(lo=n - 5, hi=n - 5)["status"] == gr.OK and run(lo=n - 4, hi=63)["status"] == gr.NO_ROOM
    r = run(lo=n - 5, hi=n - 5)                                     # exactly lo + 5: the Bars, one note, the EOS
    assert r["counts"] == (n - 5, 1, n)
    for c in (gr.EOS, gr.POSITION, gr.DURATION):                    # a class the grammar needs has no token anywhere
        gone = ci.copy()
        gone[:, c] = -1
        assert run(ci=gone)["status"] == gr.NO_ROOM
    gone = ci.copy()
    gone[:, gr.PAD] = -1                                            # without PAD the EOS is the last token of the row
    r = run(ci=gone, lo=0, hi=3)                                    # k + 4 notes + 1 == n has a solution with k in 0..3
    assert r["status"] == gr.OK and r["counts"][2] == n and r["counts"][0] + 4 * r["counts"][1] + 1 == n
    for bad in (np.nan, np.inf):
        for slot in range(7):
            hot = cs.copy()
            hot[len_meta + 3, slot] = bad
            r = run(cs=hot)
            assert r["status"] == gr.NONFINITE and np.array_equal(r["tokens"], plain)
    cold = cs.copy()
    cold[len_meta + 3, :7] = -np.inf                                # legal: every string passes through it
    cold[:len_meta] = np.nan                                        # outside the region nothing is looked at
    cold[:, 7] = np.nan
    r = run(cs=cold)
    assert r["status"] == gr.OK and r["path_score"] == -np.inf
    assert dr.decode_row(r["tokens"], mask, 2 * L, L, L, strict=True)["status"] == dr.OK


def test_forced_eos_positions_and_tie_rules():
    g = np.random.default_rng(12)
    ids, mask, cs, ci = hand_row(g, n_bars=1)
    L = len(ids)
    len_meta = L - int(mask.sum())
    n = L - len_meta
    for at in (5, n - 1):                                           # the first and the last legal place of the EOS with one Bar
        hot = cs.copy()
        hot[len_meta + at, gr.EOS] = 1000
        r = gr.constrain_row(hot, ci, ids, mask)
        assert r["status"] == gr.OK and r["counts"][2] == at + 1 and r["tokens"][len_meta + at] == 1
    # all scores equal: the first-listed predecessor wins everywhere and the smallest k at the end
    flat = np.zeros_like(cs)
    r = gr.constrain_row(flat, ci, ids, mask, lo=0, hi=5)
    assert r["status"] == gr.OK and r["counts"][0] == 0 and r["path_score"] == 0


# ------------------------------------------------------------------------------------------------------------------ class winners
def test_class_winners_restatement():
    s = np.array([[1.0, 5.0, 5.0, -np.inf, 2.0, 7.0, 7.0, 0.5]])
    cs, ci = gr.class_winners(s, ((0, 1), (1, 3), (3, 4), (4, 4), (6, 12), (9, 12), (-3, 2)))
    assert ci[0].tolist() == [0, 1, -1, -1, 6, -1, 1, 5] and cs[0, :2].tolist() == [1.0, 5.0] and cs[0, 2] == -np.inf
    assert cs[0, 4] == 7.0 and cs[0, 6] == 5.0 and cs[0, 7] == 7.0
    cs, ci = gr.class_winners(np.full((2, 4), -np.inf), gr.NOTE_CLASSES)
    assert (ci[:, :7] == -1).all() and (ci[:, 7] == 0).all() and np.isneginf(cs).all()


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_note_classes_need_no_device():
    from musediffusion_amd import ops
    from musediffusion_amd.utils import grammar_util as gu
    assert ops.note_classes() == gr.NOTE_CLASSES
    # the token ranges the decoder uses (tests/decode_ref.py)
    assert gr.NOTE_CLASSES[gr.PITCH] == (dr.PITCH0, dr.VEL0) and gr.NOTE_CLASSES[gr.VELOCITY] == (dr.VEL0, dr.CHORD0)
    assert gr.NOTE_CLASSES[gr.DURATION] == (dr.DUR0, dr.POS0) and gr.NOTE_CLASSES[gr.POSITION] == (dr.POS0, dr.BPM0)
    assert gr.NOTE_CLASSES[gr.EOS] == (dr.EOS, dr.EOS + 1) and gr.NOTE_CLASSES[gr.BAR] == (dr.BAR, dr.BAR + 1)
    assert (gu.CONSTRAIN_OK, gu.CONSTRAIN_BAD_MASK, gu.CONSTRAIN_NO_CHORDS, gu.CONSTRAIN_TOO_MANY_BARS, gu.CONSTRAIN_BAD_BOUNDS,
            gu.CONSTRAIN_NO_ROOM, gu.CONSTRAIN_NONFINITE) == tuple(range(7))
    assert len(gu.CONSTRAIN_STATUS_NAMES) == 7 and [n.upper() for n in gu.CONSTRAIN_STATUS_NAMES] == list(gr.STATUS_NAMES)
    assert _lib.lib().mhg_constrain_workspace_bytes(512, 4096) == 0
    d = gu.ConstrainResult.describe([5, 0, 1, 0, 0, 2, 0, 40, 90])
    assert d == {"rows": {"ok": 5, "bad_mask": 0, "no_chords": 1, "too_many_bars": 0, "bad_bounds": 0, "no_room": 2, "nonfinite": 0},
                 "bars": 40, "notes": 90}


def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    import torch
    from musediffusion_amd import ops, sampling
    from musediffusion_amd.utils import grammar_util as gu
    lib = _lib.lib()
    buf = (C.c_int32 * 64)()
    a = C.addressof(buf)
    assert lib.mhg_note_classes(None) == _lib.MH_ERR_INVALID and b"note_classes" in lib.mh_last_error()
    ok = dict(x=a, table=a, aux=a, classes=a, score=a, idx=a, n=1, E=4, V=4, mode=1)
    for change in (dict(x=None), dict(table=None), dict(aux=None), dict(classes=None), dict(score=None), dict(idx=None), dict(n=0), dict(n=-1),
                   dict(E=0), dict(V=0), dict(mode=0), dict(mode=3)):
        args = {**ok, **change}
        assert lib.mhg_class_argmax(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"class_argmax" in lib.mh_last_error()
    ok = dict(score=a, idx=a, ids=a, mask=a, lo=None, hi=None, policy=0, tokens=a, status=a, path=a, counts=a, ws=None, ws_bytes=0, B=1, L=8)
    for change in (dict(score=None), dict(idx=None), dict(ids=None), dict(mask=None), dict(tokens=None), dict(status=None), dict(path=None),
                   dict(counts=None), dict(B=0), dict(L=0), dict(L=4097), dict(lo=a), dict(hi=a), dict(policy=2), dict(policy=-1)):
        args = {**ok, **change}
        assert lib.mhg_constrain_rows(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"constrain_rows" in lib.mh_last_error()
    # the Python front refuses the same before it touches the library; there is no CPU path
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    with pytest.raises(_lib.MuseHipError):
        ops.class_argmax(torch.zeros(2, 4), torch.zeros(8, 4), torch.zeros(8))
    with pytest.raises(_lib.MuseHipError):
        gu.constrain_rows(torch.zeros(1, 8, 8), z(1, 8, 8), z(1, 8), z(1, 8))
    with pytest.raises(NotImplementedError, match="mid-row"):
        sampling.infill(None, None, {}, (0, 1), constrained=True)
