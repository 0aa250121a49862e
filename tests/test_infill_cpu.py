"""CPU: the infill rules without a device.  tests/infill_ref.py (the plain-Python restatement of csrc/infill.hip) on hand-made rows, one
per rule and per status; the two properties the feature is for - identity and containment - on every record of tests/golden/decode.npz
and on generated ComMU-shaped rows, judged by the decode restatement (tests/decode_ref.py); the refusals of the two entry points, which
come before any launch.  No kernel runs here: the device side is tests/test_infill_gpu.py and tests/test_infill_sampling_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as dr
import infill_ref as ir
from musediffusion_amd import _lib
from musediffusion_amd.utils import decode_util as du
from musediffusion_amd.utils import infill_util as iu
from test_decode_cpu import fixture_cases

BAR, EOS = ir.BAR, ir.EOS
Q1, Q2, Q3, Q4 = [432, 131, 3, 304], [440, 140, 60, 310], [500, 150, 70, 320], [559, 194, 130, 431]
PREFIX = [561, 602, 627, 0]                                     # m = 4
#          4     5..8  9      10..13 14..17 18     19     20..23 24
NOTES = [BAR] + Q1 + [BAR] + Q2 + Q3 + [BAR] + [BAR] + Q4 + [EOS]
TAIL = [77, 78] + [0] * 13
ROW = PREFIX + NOTES + TAIL                                     # L = 40, e = 24, bars at 4, 9, 18, 19
MASK = [0] * 4 + [1] * 36


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_status_codes_and_fields_mirror_the_header():
    assert (ir.OK, ir.NO_EOS, ir.BAD_MASK, ir.BAD_RANGE, ir.OVERFLOW) == tuple(range(5))
    assert (iu.INFILL_OK, iu.INFILL_NO_EOS, iu.INFILL_BAD_MASK, iu.INFILL_BAD_RANGE, iu.INFILL_OVERFLOW) == tuple(range(5))
    assert (iu.OK, iu.NO_EOS, iu.BAD_MASK, iu.BAD_RANGE, iu.OVERFLOW) == tuple(range(5)) and sorted(iu.STATUS_MESSAGE) == list(range(5))
    assert _lib.ABI["musehip_infill.h"].enums == {"MHI_OK": 0, "MHI_NO_EOS": 1, "MHI_BAD_MASK": 2, "MHI_BAD_RANGE": 3, "MHI_OVERFLOW": 4}
    assert iu.FIELDS == {"position": 1, "velocity": 2, "pitch": 4, "duration": 8, "all": 15}
    assert iu.field_bits("all") == 15 and iu.field_bits("pitch") == 4 and iu.field_bits(("velocity", "duration")) == 10
    assert iu.field_bits(5) == 5 and iu.field_bits(["position", "all"]) == 15
    for bad in (0, 16, -1, (), "pitches", ("pitch", "x")):
        with pytest.raises(ValueError):
            iu.field_bits(bad)
    # the re-exports, as for the encode path
    for name in ("plan_infill", "splice_infill", "InfillPlan", "InfillResult", "FIELDS", "INFILL_STATUS_MESSAGE", "INFILL_OK", "INFILL_OVERFLOW"):
        assert getattr(du, name) is getattr(iu, name)
    assert sorted(du.STATUS_MESSAGE) == list(range(8))          # the decode table is still the decode table


def test_token_classes():
    edges = {431: 3, 432: 0, 559: 0, 560: -1, 130: 2, 131: 1, 194: 1, 195: -1, 303: -1, 304: 3, 3: 2, 2: -1, 1: -1, 0: -1, -1: -1,
             729: -1, 2 ** 31 - 1: -1, -2 ** 31: -1}
    for t, c in edges.items():
        assert ir.token_class(t) == c, t
    assert [ir.token_class(t) for t in Q1] == [ir.token_class(t) for t in Q4] == [0, 1, 2, 3]


def test_plan_whole_notes_widens_the_selected_bars_and_moves_the_tail():
    out, mask, st, info = ir.plan_row(ROW, MASK, 1, 3, room=1)
    want = ROW[:18] + [0] * 4 + [BAR] + [0] * 4 + ROW[19:]     # bar 1 gets four slots behind Q2 Q3, the empty bar 2 four of its own
    assert st == ir.OK and out == want[:40] and len(want) == 48
    assert mask == [0] * 10 + [1] * 12 + [0] + [1] * 4 + [0] * 13
    assert info == (10, 27, 16, 8)
    assert out[32] == EOS and out[33:35] == [77, 78]            # the tail moved right by `added`; eight of its pads fell off
    # room 0: the row itself; BAR, the tokens before p_0, EOS and the tail are never selected
    out, mask, st, info = ir.plan_row(ROW, MASK, 0, 4)
    assert st == ir.OK and out == ROW and info == (5, 24, 16, 0)
    assert [j for j in range(40) if mask[j]] == list(range(5, 9)) + list(range(10, 18)) + list(range(20, 24))
    # the last bar ends at EOS; the empty bar has nothing to select without room
    assert ir.plan_row(ROW, MASK, 3, 4)[1] == [0] * 20 + [1] * 4 + [0] * 16
    assert ir.plan_row(ROW, MASK, 2, 3)[1:] == ([0] * 40, ir.OK, (19, 19, 0, 0))
    # tokens before the first BAR belong to no bar
    row = PREFIX + Q1 + NOTES + TAIL[:11]
    out, mask, st, info = ir.plan_row(row, MASK, 0, 1)
    assert st == ir.OK and [j for j in range(40) if mask[j]] == [9, 10, 11, 12] and info == (9, 13, 4, 0)


def test_plan_room_that_fits_exactly_and_one_slot_over():
    """the rule is e + 1 + added > L, nothing else"""
    out, mask, st, info = ir.plan_row(ROW, MASK, 0, 3, room=1)                               # 24 + 1 + 12 = 37 <= 40
    assert st == ir.OK and info == (5, 19 + 12, 12 + 12, 12)
    out, mask, st, info = ir.plan_row(ROW, MASK, 1, 4, room=1)
    assert st == ir.OK and info[3] == 12 and out[36] == EOS and out[37:] == [77, 78, 0]
    assert ir.plan_row(ROW[:37], MASK[:37], 1, 4, room=1)[2] == ir.OK                        # e + 1 + added == L
    out, mask, st, info = ir.plan_row(ROW[:36], MASK[:36], 1, 4, room=1)                     # one slot over
    assert (st, info) == (ir.OVERFLOW, (0, 0, 0, 0)) and out == ROW[:36] and mask == [0] * 36


def test_plan_every_status():
    bad = lambda r: (r[0], r[1], r[3]) == (list(ROW), [0] * 40, (0, 0, 0, 0))  # noqa: E731
    no_eos = [t if t != EOS else 5 for t in ROW]
    r = ir.plan_row(no_eos, MASK, 0, 1)
    assert r[2] == ir.NO_EOS and r[0] == no_eos
    eos_in_prefix = list(no_eos)
    eos_in_prefix[2] = EOS                                       # an EOS in front of m does not count
    assert ir.plan_row(eos_in_prefix, MASK, 0, 1)[2] == ir.NO_EOS
    for mask in ([0] * 40, [1] * 40, [0] * 4 + [1] * 35 + [0], [0] * 4 + [1, 2] + [1] * 34, [0, 1, 0, 0] + [1] * 36, [0] * 4 + [-1] * 36):
        r = ir.plan_row(ROW, mask, 0, 1)
        assert r[2] == ir.BAD_MASK and bad(r), mask
    for lo, hi in ((-1, 1), (0, 5), (2, 2), (3, 2), (4, 5), (0, 0), (-2 ** 31, 2 ** 31 - 1)):
        r = ir.plan_row(ROW, MASK, lo, hi)
        assert r[2] == ir.BAD_RANGE and bad(r), (lo, hi)
    r = ir.plan_row(ROW, MASK, 0, 4, room=1)
    assert r[2] == ir.OVERFLOW and bad(r)
    no_bar = PREFIX + Q1 + [EOS] + [0] * 31
    assert ir.plan_row(no_bar, MASK, 0, 1)[2] == ir.BAD_RANGE     # nb = 0: no range is valid
    # the order: the mask first, then the EOS, then the range, then the room
    assert ir.plan_row(no_eos, [1] * 40, 9, 9)[2] == ir.BAD_MASK and ir.plan_row(no_eos, MASK, 9, 9)[2] == ir.NO_EOS
    assert ir.plan_row(ROW, MASK, 0, 5, room=99)[2] == ir.BAD_RANGE


def test_plan_fields_selects_only_whole_quads_inside_one_interior():
    for bits in range(1, 15):
        out, mask, st, info = ir.plan_row(ROW, MASK, 1, 4, fields=bits)
        want = [j for q in (10, 14, 20) for c in range(4) if bits >> c & 1 for j in [q + c]]
        assert st == ir.OK and out == ROW and sorted(want) == [j for j in range(40) if mask[j]] and info == (10, 24, len(want), 0)
    # malformed quads: a lone position, velocity and pitch swapped, a quad cut by the bar end, a quad cut by EOS
    body = [BAR, 432, 432, 131, 3, 304, 432, 3, 131, 304, 432, 131, 3, BAR, 304, 432, 131, 3, EOS]
    row = PREFIX + body + [304] + [0] * 16
    mask = ir.plan_row(row, MASK, 0, 2, fields=14)[1]
    assert [j for j in range(40) if mask[j]] == [7, 8, 9]        # of 5 (pos) 6..9 the quad: its velocity, pitch, duration
    mask = ir.plan_row(row, MASK, 0, 2, fields=1)[1]
    assert [j for j in range(40) if mask[j]] == [6]
    assert sum(ir.plan_row(row, MASK, 1, 2, fields=15 - 8)[1]) == 0   # 432 131 3 EOS 304: the duration lies behind the EOS
    with pytest.raises(AssertionError):
        ir.plan_row(ROW, MASK, 0, 1, room=1, fields=4)


def test_splice_whole_notes_keeps_whole_quads_only():
    ptok, pmask, st, info = ir.plan_row(ROW, MASK, 1, 3, room=1)
    junk = [9999 - j for j in range(40)]
    region = [j for j in range(40) if pmask[j]]
    assert region == list(range(10, 22)) + list(range(23, 27))

    def run(fill):
        s = list(junk)
        for j, v in zip(region, fill):
            s[j] = v
        return ir.splice_row(s, ptok, pmask, st)
    # the identity: the plan's own tokens come back as the original row
    assert run([ptok[j] for j in region]) == (ROW, (8, 8, 0, 0))
    # all pads: the bars are emptied, the rest closes up
    out, counts = run([0] * 16)
    assert out == ROW[:10] + ROW[18:] + [0] * 8 and counts == (0, 16, 0, 0)
    # no pads: four notes where two were
    out, counts = run(Q4 + Q3 + Q2 + Q1)
    assert out == (ROW[:10] + Q4 + Q3 + Q2 + [BAR] + Q1 + ROW[19:])[:40] and counts == (16, 0, 0, 0) and out[32] == EOS
    # alternating pads: the quads close up over them, also across what were two different gaps
    out, counts = run([0, 440, 0, 140, 0, 60, 0, 310, 0, 0, 0, 0, 500, 150, 70, 320])
    assert out == ROW[:10] + Q2 + [BAR] + Q3 + ROW[19:] and counts == (8, 8, 0, 0)
    # stray BAR / EOS, negatives, out-of-vocabulary tokens, a chord token: dropped as other, and what they cut apart closes up
    out, counts = run([440, BAR, 140, EOS, 60, -7, 310, 729, 200, 2 ** 31 - 1, 0, 0, 0, 0, 0, 0])
    assert out == ROW[:10] + Q2 + ROW[18:] + [0] * 4 and counts == (4, 6, 6, 0)
    # a half quad at the end of a bar does not borrow from the next bar, one at its start not from the BAR's other side
    out, counts = run(Q2 + [500, 150, 70] + [0] * 5 + [320, 500, 150, 70])
    assert out == ROW[:10] + Q2 + ROW[18:] + [0] * 4 and counts == (4, 5, 7, 0)
    # three tokens in an otherwise empty bar: nothing to borrow from either BAR
    out, counts = run([0] * 12 + [0, 559, 194, 130])
    assert out == ROW[:10] + [BAR, BAR] + ROW[20:] + [0] * 8 and counts == (0, 13, 3, 0)
    # region tokens do not pair with anchored ones: under a hand-made mask over Q2's first three tokens its anchored duration stays alone
    hand = [1 if j in (10, 11, 12) else 0 for j in range(40)]
    assert ir.splice_row(ROW, ROW, hand, ir.OK) == (ROW[:10] + [310] + ROW[14:] + [0] * 3, (0, 0, 3, 0))
    # a row that was not planned comes back as it is, whatever was sampled
    assert ir.splice_row(junk, ROW, [1] * 40, ir.NO_EOS) == (ROW, (0, 0, 0, 0))


def test_splice_fields_takes_tokens_of_the_same_class_only():
    ptok, pmask, st, _ = ir.plan_row(ROW, MASK, 1, 2, fields=4 | 1)
    assert [j for j in range(40) if pmask[j]] == [10, 12, 14, 16]
    s = [-5] * 40
    s[10], s[12], s[14], s[16] = 433, 61, 500, 200              # a new position, a new pitch, the same position, a chord for a pitch
    out, counts = ir.splice_row(s, ptok, pmask, st, fields=5)
    want = list(ROW)
    want[10], want[12] = 433, 61
    assert out == want and counts == (3, 0, 1, 2)
    s[12] = 131                                                  # a velocity where a pitch belongs
    assert ir.splice_row(s, ptok, pmask, st, fields=5)[1] == (2, 0, 2, 1)


# ------------------------------------------------------------------------------------------------------------------ the properties
def _note_bars(r):
    """bar of every note of a decoded row: start // ticks_per_bar, less one when the restored row does not begin with BAR"""
    tpb = 480 * dr.BEATS[int(r["meta"][2]) - 627]
    shift = 0 if len(r["restored"]) and r["restored"][0] == BAR else 1
    return [int(n[0]) // tpb - shift for n in r["notes"]]


def _outside(r, lo, hi):
    return [tuple(int(x) for x in n) for n, k in zip(r["notes"], _note_bars(r)) if not lo <= k < hi]


def _chords_outside(r, lo, hi):
    """the chord markers of the other bars (those of a regenerated bar follow its new positions: restore_chord places them by position)"""
    tpb = 480 * dr.BEATS[int(r["meta"][2]) - 627]
    shift = 0 if len(r["restored"]) and r["restored"][0] == BAR else 1
    return [(int(t), int(c)) for t, c in r["chords"] if not lo <= int(t) // tpb - shift < hi]


def _decode(tokens, mask, strict):
    return dr.decode_row(tokens, mask, dr.MAX_ROW, 2048, 2048, strict)


def _rows():
    """(name, tokens, mask): the fixture's records, and generated rows with spare room behind the EOS"""
    out = [(c.name, np.asarray(c.tokens, np.int64), np.asarray(c.mask, np.int64)) for c in fixture_cases()]
    g = np.random.default_rng(41)
    for kind in ("clean", "extra_bar", "two_extra_bars"):
        for n in range(4):
            t, m = dr.make_row(g, 320 if n < 3 else 1024, kind)
            out.append(("%s_%d" % (kind, n), t.astype(np.int64), m.astype(np.int64)))
    return out


def _ranges(nb):
    return sorted({(0, 1), (nb - 1, nb), (0, nb), (max(nb // 2 - 1, 0), nb // 2 + 1)}) if nb >= 1 else [(0, 1)]


def _hostile_fill(g, n):
    """n region tokens: note tokens of every class, pads, BAR, EOS, out-of-range values, and some planted whole quads"""
    if n == 0:
        return np.zeros(0, np.int64)
    pool = np.concatenate([g.integers(3, 560, size=n), np.zeros(n, np.int64), np.full(n, BAR), np.full(n, EOS),
                           g.choice([-1, -9, 560, 729, 1000, 2 ** 31 - 1, -2 ** 31, 195, 303], size=n)])
    w = np.concatenate([np.full(n, 0.55), np.full(n, 0.25), np.full(n, 0.05), np.full(n, 0.05), np.full(n, 0.10)]) / n
    fill = g.choice(pool, size=n, p=w / w.sum())
    for _ in range(max(1, n // 12)):
        if n >= 4:
            at = int(g.integers(0, n - 3))
            fill[at:at + 4] = [int(g.integers(432, 560)), int(g.integers(131, 195)), int(g.integers(3, 131)), int(g.integers(304, 432))]
    return fill


def test_identity_and_containment_on_the_fixture_and_on_generated_rows():
    g = np.random.default_rng(97)
    identity = containment = planned = widened = overflowed = 0
    for name, tokens, mask in _rows():
        L = len(tokens)
        orig = {s: _decode(tokens, mask, s) for s in (False, True)}
        if orig[True]["status"] != dr.OK:
            continue
        st, m, e, bars = ir.layout(tokens, mask)
        assert st == ir.OK, name                                  # a row that decodes strictly has a mask, an EOS and bars
        for lo, hi in _ranges(len(bars)):
            for room in (0, 1, 3):
                ptok, pmask, pst, info = ir.plan_row(tokens, mask, lo, hi, room)
                if not bars:                                      # a piece without a BAR has no bar to regenerate: it comes back as it is
                    assert pst == ir.BAD_RANGE, name
                else:
                    assert pst in (ir.OK, ir.OVERFLOW), (name, lo, hi, room)
                    assert pst == ir.OK or (room > 0 and e + 1 + 4 * room * (hi - lo) > L)
                planned += pst == ir.OK
                widened += pst == ir.OK and room > 0
                overflowed += pst == ir.OVERFLOW
                # identity
                if not np.any(tokens[e + 1:]):
                    out, counts = ir.splice_row(ptok, ptok, pmask, pst)
                    assert out == tokens.tolist(), (name, lo, hi, room)
                    assert counts[0] % 4 == 0 and sum(counts[:3]) == info[2] and counts[2] == 0 and counts[1] >= info[3]
                    identity += 1
                # containment: hostile tokens in the region, junk everywhere else
                sampled = g.integers(-5, 800, size=L)
                region = [j for j in range(L) if pmask[j]]
                sampled[region] = _hostile_fill(g, len(region))
                out, counts = ir.splice_row(sampled, ptok, pmask, pst)
                assert counts[0] % 4 == 0 and sum(counts[:3]) == info[2] and counts[3] == 0
                for strict in (False, True):
                    r = _decode(out, mask, strict)
                    assert r["status"] in (dr.OK, dr.ONCE_FAILED), (name, lo, hi, room, strict, r["status"])
                    if r["status"] == dr.OK:
                        assert _outside(r, lo, hi) == _outside(orig[strict], lo, hi), (name, lo, hi, room, strict)
                        assert _chords_outside(r, lo, hi) == _chords_outside(orig[strict], lo, hi), (name, lo, hi, room, strict)
                    containment += 1
    print("identity %d, containment %d, planned %d (widened %d), overflow %d" % (identity, containment, planned, widened, overflowed))
    assert identity > 300 and containment > 600 and widened > 50 and overflowed > 50


def test_field_mode_keeps_every_other_field_of_every_note():
    g = np.random.default_rng(5)
    checked = 0
    for name, tokens, mask in _rows():
        orig = _decode(tokens, mask, True)
        if orig["status"] != dr.OK:
            continue
        nb = len(ir.layout(tokens, mask)[3])
        if nb == 0:
            continue
        for lo, hi in _ranges(nb):
            for bits in (4, 5, 14):
                ptok, pmask, pst, info = ir.plan_row(tokens, mask, lo, hi, 0, bits)
                assert pst == ir.OK and ptok == tokens.tolist()
                sampled = g.integers(3, 560, size=len(tokens))     # any note token anywhere: about a quarter have the slot's class
                out, counts = ir.splice_row(sampled, ptok, pmask, pst, bits)
                assert counts[0] + counts[2] == info[2] and counts[1] == 0 and counts[3] <= counts[0]
                diff = [j for j in range(len(tokens)) if out[j] != tokens[j]]
                assert len(diff) == counts[3] and all(pmask[j] and ir.token_class(out[j]) == ir.token_class(tokens[j]) for j in diff)
                assert all((bits >> ir.token_class(tokens[j])) & 1 for j in diff)
                r = _decode(out, mask, True)
                assert r["status"] == dr.OK, (name, lo, hi, bits)
                if not bits & 1:                                   # positions untouched: restore_chord and the bars see the same row
                    assert len(r["notes"]) == len(orig["notes"]) and _note_bars(r) == _note_bars(orig)
                    assert _outside(r, lo, hi) == _outside(orig, lo, hi) and np.array_equal(r["chords"], orig["chords"])
                    # columns: start, end (start + duration), pitch, velocity
                    same = [0] + [col for col, bit in ((1, 8), (2, 4), (3, 2)) if not bits & bit]
                    assert np.array_equal(r["notes"][:, same], orig["notes"][:, same]), (name, lo, hi, bits)
                checked += 1
    assert checked > 100


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID and a text"""
    lib = _lib.lib()
    buf = (C.c_int32 * 64)()
    a = C.addressof(buf)
    max_row = lib.mh_batch_max_row()
    assert max_row == 4096
    ok = dict(tokens=a, pmask=a, lo=a, hi=a, room=0, fields=15, otok=a, omask=a, status=a, info=a, B=1, L=8)
    bad = [dict(tokens=None), dict(pmask=None), dict(lo=None), dict(hi=None), dict(otok=None), dict(omask=None), dict(status=None),
           dict(info=None), dict(B=0), dict(B=-3), dict(L=0), dict(L=-1), dict(L=max_row + 1), dict(room=-1), dict(fields=0), dict(fields=16),
           dict(fields=-1), dict(fields=4, room=1), dict(fields=14, room=2)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhi_infill_plan(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"infill_plan" in lib.mh_last_error()
    ok = dict(sampled=a, ptok=a, pmask=a, status=a, fields=15, out=a, counts=a, B=1, L=8)
    bad = [dict(sampled=None), dict(ptok=None), dict(pmask=None), dict(status=None), dict(out=None), dict(counts=None), dict(B=0), dict(L=0),
           dict(L=max_row + 1), dict(fields=0), dict(fields=16)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhi_infill_splice(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"infill_splice" in lib.mh_last_error()
    # the Python front refuses the same before it touches a tensor
    for kw in (dict(room=-1), dict(room=1, fields="pitch"), dict(fields=0), dict(fields="tempo")):
        with pytest.raises(ValueError):
            iu.plan_infill(None, None, (0, 1), **kw)
