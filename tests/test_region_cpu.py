"""Region-constrained rounding without a device: the restatement tests/region_ref.py against brute-force enumeration of every accepted
string of every segment, every status on hand-made rows, the restatement's output through the splice restatement (tests/infill_ref.py:
nothing but pads is dropped), the refusals."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as dr
import infill_ref as ir
import region_ref as rr
from musediffusion_amd import _lib
from test_decode_cpu import fixture_cases

CLASS_RANGE = {rr.PAD: (0, 1), rr.PITCH: (3, 131), rr.VELOCITY: (131, 195), rr.DURATION: (304, 432), rr.POSITION: (432, 560)}


def int_tables(g, n, lo=-8, hi=8, gone=0.0):
    """integer scores (exact in fp32, sums too; a narrow range plants ties) and per-slot tokens of the ComMU classes; slot 7, EOS and
    BAR hold tokens the region grammar never emits; `gone`: the share of used slots without a token"""
    cs = g.integers(lo, hi + 1, (n, 8)).astype(np.float32)
    ci = np.zeros((n, 8), np.int32)
    for c, (a, b) in CLASS_RANGE.items():
        ci[:, c] = g.integers(a, b, n)
    ci[:, rr.EOS], ci[:, rr.BAR], ci[:, rr.ANY] = 1, 2, g.integers(560, 729, n)
    if gone:
        for c in rr.USED:
            ci[g.random(n) < gone, c] = -1
    return cs, ci


def tie_key(s):
    """the order the tie rule puts on strings of one score: read from the END, at every arrival in S a note goes before a pad"""
    key, t = [], len(s) - 1
    while t >= 0:
        if s[t] == rr.PAD:
            key.append(1)
            t -= 1
        else:
            key.append(0)
            t -= 4
    return key


# ------------------------------------------------------------------------------------------------------------------ brute force
def test_accepted_strings_are_the_grammar():
    counts = [len(rr.accepted_strings(n)) for n in range(13)]
    assert counts[:5] == [1, 1, 1, 1, 2]
    assert all(counts[n] == counts[n - 1] + counts[n - 4] for n in range(4, 13))
    for n in (0, 3, 4, 9, 12):
        strings = rr.accepted_strings(n)
        assert len({tuple(s) for s in strings}) == len(strings)
        for s in strings:
            assert len(s) == n
            i = 0
            while i < n:
                if s[i] == rr.PAD:
                    i += 1
                else:
                    assert s[i:i + 4] == list(rr.QUAD), s
                    i += 4


def test_restatement_equals_brute_force_on_tiny_segments():
    g = np.random.default_rng(1)
    tied = no_room = checked = 0
    for case in range(600):
        n = int(g.integers(1, 13))
        cs, ci = int_tables(g, n, *((-2, 2) if case % 3 == 0 else (-8, 8)), gone=(0.0, 0.0, 0.08)[case % 3])
        classes, total, notes, pads = rr.viterbi_segment(cs, ci)
        best, score = rr.brute_force(cs, ci)
        if not best:
            assert classes is None, case
            no_room += 1
            continue
        assert classes is not None and float(total) == score, (case, total, score)
        assert tuple(classes) == min(best, key=tie_key), (case, classes, best)     # the maximum, and among equals the tie rule's
        assert notes == classes.count(rr.DURATION) and pads == classes.count(rr.PAD) and 4 * notes + pads == n
        tied += len(best) > 1
        checked += 1
    print("brute force: %d checked, %d of them tied, %d without room" % (checked, tied, no_room))
    assert checked >= 300 and tied >= 30 and no_room >= 10


def test_brute_force_on_whole_rows_with_several_segments():
    """rows of a few short segments: the row's score is the segments' sum in order, its tokens the segments' strings side by side"""
    g = np.random.default_rng(2)
    for case in range(300):
        L = int(g.integers(1, 25))
        mask = (g.random(L) < 0.7).astype(np.int32)
        mask[g.random(L) < 0.1] = (2, -1)[case % 2]                    # neither counts as masked
        cs, ci = int_tables(g, L, -4, 4)
        r = rr.constrain_row(cs, ci, np.zeros(L, np.int32), mask, 0)
        segs = rr.segments([m == 1 for m in mask])
        assert r["status"] == rr.OK and r["counts"][0] == int((mask == 1).sum()) and r["counts"][3] == len(segs)
        total, want = 0.0, ci[:, rr.ANY].copy()
        for start, n in segs:
            best, score = rr.brute_force(cs[start:start + n], ci[start:start + n])
            total += score
            pick = min(best, key=tie_key)
            want[start:start + n] = ci[np.arange(start, start + n), list(pick)]
        assert float(r["path_score"]) == total and np.array_equal(r["tokens"], want), case


# ------------------------------------------------------------------------------------------------------------------ statuses
def test_every_status_on_hand_made_rows():
    g = np.random.default_rng(3)
    L = 24
    cs, ci = int_tables(g, L)
    plain = ci[:, rr.ANY]
    ptok = np.array([5] * 4 + [2] + [432, 131, 3, 304] * 2 + [2] + [440, 140, 60, 310] + [1] + [0] * 5, np.int32)
    mask = np.array([0] * 5 + [1] * 8 + [0] + [1] * 4 + [0] * 6, np.int32)
    run = lambda **kw: rr.constrain_row(kw.pop("cs", cs), kw.pop("ci", ci), kw.pop("ptok", ptok), kw.pop("mask", mask),  # noqa: E731
                                        kw.pop("status", 0), **kw)
    left = lambda r: np.array_equal(r["tokens"], plain) and r["counts"] == (0, 0, 0, 0) and r["path_score"] == 0  # noqa: E731
    r = run()
    assert r["status"] == rr.OK and r["counts"][0] == 12 and r["counts"][3] == 2 and 4 * r["counts"][1] + r["counts"][2] == 12
    assert np.array_equal(r["tokens"][mask == 0], plain[mask == 0])
    # a worked answer: a note that pays in the first four slots of the first segment, pads that pay everywhere else
    easy = np.zeros((L, 8), np.float32)
    easy[5:9, [rr.POSITION, rr.VELOCITY, rr.PITCH, rr.DURATION]] = np.eye(4, dtype=np.float32) * 3
    easy[9:, rr.PAD] = 1
    r = run(cs=easy)
    assert r["status"] == rr.OK and r["counts"] == (12, 1, 8, 2) and r["path_score"] == 12 + 8
    assert r["tokens"][5:9].tolist() == [ci[5, rr.POSITION], ci[6, rr.VELOCITY], ci[7, rr.PITCH], ci[8, rr.DURATION]]
    assert not r["tokens"][9:13].any() and not r["tokens"][14:18].any()
    # all scores equal: ties go to the note, from the end of every segment
    r = run(cs=np.zeros((L, 8), np.float32))
    assert r["counts"] == (12, 3, 0, 2) and r["path_score"] == 0
    for st in (1, 4, -1):
        r = run(status=st)
        assert r["status"] == rr.NOT_PLANNED and left(r)
    # field mode: the slot of the plan token's class; a masked token of class -1 is a bad plan - in field mode only
    fmask = np.array([0] * 5 + [0, 0, 1, 0] * 2 + [0] + [0, 0, 1, 0] + [0] * 6, np.int32)
    r = run(mask=fmask, fields=4)
    assert r["status"] == rr.OK and r["counts"] == (3, 0, 0, 3) and r["tokens"][[7, 11, 16]].tolist() == ci[[7, 11, 16], rr.PITCH].tolist()
    assert r["path_score"] == np.float32(cs[7, rr.PITCH] + cs[11, rr.PITCH]) + cs[16, rr.PITCH]
    r = run(mask=mask, fields=14)                                      # every class: position slots too, whatever the bits say
    assert r["status"] == rr.OK and r["tokens"][5] == ci[5, rr.POSITION] and r["tokens"][8] == ci[8, rr.DURATION] and r["counts"] == (12, 0, 0, 2)
    hostile = fmask.copy()
    hostile[4] = 1                                                     # the BAR under the mask
    r = run(mask=hostile, fields=4)
    assert r["status"] == rr.BAD_PLAN and left(r)
    assert run(mask=hostile)["status"] == rr.OK                        # whole notes do not look at the plan's tokens
    # NaN / +inf in a used slot of a masked position; -inf, the other slots and the unmasked positions are not looked at
    for bad in (np.nan, np.inf):
        for slot in rr.USED:
            hot = cs.copy()
            hot[16, slot] = bad
            for kw in (dict(), dict(mask=fmask, fields=4)):
                r = run(cs=hot, **kw)
                assert r["status"] == rr.NONFINITE and left(r), (bad, slot)
        hot = cs.copy()
        hot[16, [rr.EOS, rr.BAR, rr.ANY]] = bad
        hot[13] = bad
        hot[:5] = bad
        assert run(cs=hot)["status"] == rr.OK
    assert run(cs=hot, mask=hostile, fields=4)["status"] == rr.BAD_PLAN  # the order of the header
    cold = cs.copy()
    cold[6, :] = -np.inf
    r = run(cs=cold)
    assert r["status"] == rr.OK and r["path_score"] == -np.inf
    # no room: without PAD a segment must be whole notes; one quad class without a token leaves pads only
    gone = ci.copy()
    gone[:, rr.PAD] = -1
    r = run(ci=gone)
    assert r["status"] == rr.OK and r["counts"] == (12, 3, 0, 2)
    odd = mask.copy()
    odd[17] = 0
    r = run(ci=gone, mask=odd)
    assert r["status"] == rr.NO_ROOM and left(r)
    for c in rr.QUAD:
        gone = ci.copy()
        gone[:, c] = -1
        assert run(ci=gone)["counts"] == (12, 0, 12, 2)
        gone[9, rr.PAD] = -1
        assert run(ci=gone)["status"] == rr.NO_ROOM
    gone = ci.copy()
    gone[11, rr.PITCH] = -1
    r = run(ci=gone, mask=fmask, fields=4)
    assert r["status"] == rr.NO_ROOM and left(r)
    gone[11, rr.PITCH], gone[11, rr.POSITION] = 9, -1                  # another slot of that position: not read
    assert run(ci=gone, mask=fmask, fields=4)["status"] == rr.OK
    hot = cs.copy()
    hot[16, rr.PAD] = np.nan
    assert run(cs=hot, ci=gone, mask=odd)["status"] == rr.NONFINITE    # NONFINITE before NO_ROOM
    r = run(mask=np.zeros(L, np.int32))                                # nothing masked: OK, and nothing to do
    assert r["status"] == rr.OK and left(r)


# ------------------------------------------------------------------------------------------------------------------ through the splice
def random_tables(g, L, pad_bias=0.0, gone=0.0):
    cs, ci = int_tables(g, L, gone=gone)
    cs = (g.standard_normal((L, 8)) * 2).astype(np.float32)
    cs[:, rr.PAD] += np.float32(pad_bias)
    top = np.where(ci[:, :7] >= 0, cs[:, :7], -np.inf).argmax(1)
    ci[:, rr.ANY] = ci[np.arange(L), top]                              # slot 7: the plain argmax, a token of ANY class per slot
    return cs, ci


def check_through_splice(cs, ci, ptok, pmask, pstat, fields, what):
    """-> (the restatement's row, the splice's counts); on an OK row nothing but pads is dropped"""
    r = rr.constrain_row(cs, ci, ptok, pmask, pstat, fields)
    out, (kept, pads, other, changed) = ir.splice_row(r["tokens"], ptok, pmask, pstat, fields)
    if r["status"] == rr.OK and pstat == ir.OK:
        masked, notes, placed, segs = r["counts"]
        assert other == 0, what
        if fields == rr.ALL:
            assert kept == 4 * notes and pads == placed and kept + pads == masked, what
        else:
            assert kept == masked and pads == 0, what                  # rejected is `other` in field mode: 0
    return r, (kept, pads, other, changed)


def test_restatement_through_the_splice_restatement():
    g = np.random.default_rng(7)
    lost = rows = 0
    for case in range(60):
        L = (96, 160, 320)[case % 3]
        ids, mask = dr.make_row(g, L, ("clean", "extra_bar", "two_extra_bars")[case % 3], n_bars=1 + case % 4, notes_per_bar=2)
        st, m, e, bars = ir.layout(ids, mask)
        assert st == ir.OK
        nb = len(bars)
        for lo, hi in sorted({(0, 1), (nb - 1, nb), (0, nb)}):
            for room, fields in ((0, 15), (2, 15), (0, 4), (0, 11), (0, 14)):
                ptok, pmask, pstat, info = ir.plan_row(ids, mask, lo, hi, room, fields)
                cs, ci = random_tables(g, L, pad_bias=(0.0, 2.0)[case % 2], gone=(0.0, 0.03)[case // 3 % 2] if fields == 15 else 0.0)
                r, counts = check_through_splice(cs, ci, ptok, pmask, pstat, fields, (case, lo, hi, room, fields))
                if pstat != ir.OK:
                    assert r["status"] == rr.NOT_PLANNED
                    continue
                assert r["status"] in (rr.OK, rr.NO_ROOM)
                if r["status"] != rr.OK:
                    continue
                rows += 1
                assert r["counts"][0] == info[2]
                # the plain argmax on the same tables loses tokens the region rounding keeps
                plain_out, plain = ir.splice_row(ci[:, rr.ANY], ptok, pmask, pstat, fields)
                lost += plain[2]
    print("through the splice: %d OK rows; the plain argmax lost %d tokens on them, the region rounding none" % (rows, lost))
    assert rows > 500 and lost > 1000


def test_same_property_on_planned_fixture_rows():
    g = np.random.default_rng(8)
    planned = not_planned = 0
    for c in fixture_cases():
        ids, mask = np.asarray(c.tokens, np.int64), np.asarray(c.mask, np.int64)
        L = len(ids)
        if L > 700:                                                    # the 2096-token record: its shape adds nothing here
            continue
        st, m, e, bars = ir.layout(ids, mask)
        nb = len(bars) if st == ir.OK else 0
        for lo, hi in sorted({(0, 1), (max(nb - 1, 0), max(nb, 1)), (0, max(nb, 1))}):
            for room, fields in ((0, 15), (1, 15), (0, 6)):
                ptok, pmask, pstat, info = ir.plan_row(ids, mask, lo, hi, room, fields)
                cs, ci = random_tables(g, L)
                r, counts = check_through_splice(cs, ci, ptok, pmask, pstat, fields, (c.name, lo, hi, room, fields))
                if pstat == ir.OK:
                    assert r["status"] == rr.OK, (c.name, r["status"])
                    planned += 1
                else:
                    assert r["status"] == rr.NOT_PLANNED and counts == (0, 0, 0, 0)
                    not_planned += 1
    assert planned > 100 and not_planned > 0


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_python_mirrors_need_no_device():
    from musediffusion_amd.utils import grammar_util as gu
    assert (gu.REGION_OK, gu.REGION_NOT_PLANNED, gu.REGION_BAD_PLAN, gu.REGION_NONFINITE, gu.REGION_NO_ROOM) == tuple(range(5))
    assert [n.upper() for n in gu.REGION_STATUS_NAMES] == list(rr.STATUS_NAMES)
    d = gu.RegionResult.describe([5, 1, 0, 0, 2, 64, 12, 16, 9])
    assert d == {"rows": {"ok": 5, "not_planned": 1, "bad_plan": 0, "nonfinite": 0, "no_room": 2}, "masked": 64, "notes": 12, "pads": 16,
                 "segments": 9}
    for c, slot in rr.FIELD_SLOT.items():                              # infill class -> the class range of that slot
        lo, hi = CLASS_RANGE[slot]
        assert ir.token_class(lo) == ir.token_class(hi - 1) == c


def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text that names the entry point"""
    import torch
    from types import SimpleNamespace
    from musediffusion_amd import sampling
    from musediffusion_amd.utils import grammar_util as gu
    lib = _lib.lib()
    buf = (C.c_int32 * 64)()
    a = C.addressof(buf)
    ok = dict(score=a, idx=a, ptok=a, pmask=a, pstat=a, fields=15, tokens=a, status=a, path=a, counts=a, B=1, L=8)
    for change in (dict(score=None), dict(idx=None), dict(ptok=None), dict(pmask=None), dict(pstat=None), dict(tokens=None), dict(status=None),
                   dict(path=None), dict(counts=None), dict(B=0), dict(B=-1), dict(L=0), dict(L=4097), dict(fields=0), dict(fields=16),
                   dict(fields=-1)):
        args = {**ok, **change}
        assert lib.mhr_constrain_regions(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"constrain_regions" in lib.mh_last_error(), change
    # the Python front refuses the same before it touches the library; there is no CPU path
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    plan = SimpleNamespace(tokens=z(1, 8), mask=z(1, 8), status=z(1), fields=15)
    with pytest.raises(_lib.MuseHipError):
        gu.constrain_regions(torch.zeros(1, 8, 8), z(1, 8, 8), plan)
    with pytest.raises(ValueError, match="rounding"):
        sampling.infill(None, None, {}, (0, 1), rounding="viterbi")
    with pytest.raises(ValueError, match="rounding"):
        sampling.run_infill(None, None, [], bars=(0, 1), step=1, batch_size=1, rounding="viterbi")
    with pytest.raises(NotImplementedError, match="mid-row"):
        sampling.infill(None, None, {}, (0, 1), constrained=True, rounding="region")
