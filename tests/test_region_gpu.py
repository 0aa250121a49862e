"""GPU: mhr_constrain_regions (csrc/region.hip) through the C ABI (include/musehip_region.h), outputs sentinel-filled between guard
bands, bit for bit against the restatement tests/region_ref.py - on mhg_class_argmax's own tables of random hidden states and on
injected integer tables; masks built for the seams of the kernel (64-lane ballots, 256-position chunks, the stride over the segment
table, two segments one slot apart); real plans from mhi_infill_plan and mhi_infill_splice on the output: nothing but pads is dropped."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import infill_ref as ir  # noqa: E402
import region_ref as rr  # noqa: E402
from gpu_helpers import Guarded, library_launches  # noqa: E402
from musediffusion_amd import _lib, ops  # noqa: E402
from musediffusion_amd.utils import grammar_util as gu  # noqa: E402
from test_grammar_gpu import SENT_F, f32, i32, same  # noqa: E402
from test_infill_gpu import plan as device_plan, random_batch, splice as device_splice  # noqa: E402
from test_region_cpu import CLASS_RANGE  # noqa: E402

DEV = "cuda"
LENGTHS = (1, 2, 3, 4, 5, 8, 63, 64, 65, 255, 256, 257)


def run_regions(cs, ci, ptok, pmask, pstat, fields=15):
    """mhr_constrain_regions through the C ABI -> dict of numpy arrays, as region_ref.constrain_rows; cs / ci [B, L, 8] host or device"""
    B, L = ptok.shape
    csd = cs if isinstance(cs, torch.Tensor) else f32(cs)
    cid = ci if isinstance(ci, torch.Tensor) else i32(ci)
    t, m, s = i32(ptok), i32(pmask), i32(pstat)
    out = dict(tokens=Guarded(B, L), status=Guarded(B), path_score=Guarded(B, dtype=torch.float32, sentinel=SENT_F),
               counts=Guarded(B, 4))
    _lib.check(_lib.lib().mhr_constrain_regions(csd.data_ptr(), cid.data_ptr(), t.data_ptr(), m.data_ptr(), s.data_ptr(), fields,
                                                out["tokens"].ptr, out["status"].ptr, out["path_score"].ptr, out["counts"].ptr, B, L,
                                                _lib.current_stream()), "mhr_constrain_regions")
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}


def check(cs, ci, ptok, pmask, pstat=None, fields=15, what=""):
    pstat = np.zeros(len(ptok), np.int32) if pstat is None else pstat
    got = run_regions(cs, ci, ptok, pmask, pstat, fields)
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t  # noqa: E731
    same(got, rr.constrain_rows(host(cs), host(ci), ptok, pmask, pstat, fields), what)
    return got


def int_tables(g, B, L, pad_bias=0):
    """integer scores in [-64, 64] (sums exact in fp32) and per-slot tokens of the ComMU classes; slot 7 is junk of its own"""
    cs = g.integers(-64, 65, (B, L, 8)).astype(np.float32)
    cs[:, :, rr.PAD] += pad_bias
    ci = np.zeros((B, L, 8), np.int32)
    for c, (lo, hi) in CLASS_RANGE.items():
        ci[:, :, c] = g.integers(lo, hi, (B, L))
    ci[:, :, rr.EOS], ci[:, :, rr.BAR], ci[:, :, rr.ANY] = 1, 2, g.integers(560, 729, (B, L))
    return cs, ci


def own_tables(g, B, L, E=16, V=729):
    """mhg_class_argmax's tables of random hidden states against a random head: they stay on the device"""
    W, b = f32(0.5 * g.standard_normal((V, E))), np.zeros(V, np.float32)
    b[0] = 1.0                                                          # a head that likes PAD a little, so that both kinds of S arrival occur
    cs, ci = ops.class_argmax(f32(g.standard_normal((B * L, E))), W, f32(b), 1)
    return cs.view(B, L, 8), ci.view(B, L, 8)


def segments_mask(L, segs):
    m = np.zeros(L, np.int32)
    for start, n in segs:
        assert 0 <= start and start + n <= L
        m[start:start + n] = 1
    return m


def seam_masks(L):
    """the masks at which the kernel can go wrong, as rows [L]"""
    rows = []
    # every length that fits, one slot apart (two threads' decision bytes side by side), from position 0 and from position 1
    for first in (0, 1):
        segs, at = [], first
        for n in LENGTHS + LENGTHS[::-1]:
            if at + n <= L:
                segs.append((at, n))
                at += n + 1
        rows.append(segments_mask(L, segs))
    # segments that begin and end on the 64 and 256 seams, and one slot either side of them
    for d0, d1 in ((0, 0), (-1, 1), (1, -1), (0, 1), (-1, 0)):
        segs = []
        for a, b in ((64, 128), (192, 256), (256, 512), (576, 640), (768, 1024), (1280, 1281)):
            if b + 1 < L:
                segs.append((a + d0, b + d1 - a - d0))
        if segs:
            rows.append(segments_mask(L, segs))
    rows.append(segments_mask(L, [(1, L - 2)]))                         # one of L - 2
    rows.append(segments_mask(L, [(0, L)]))                             # the whole row
    rows.append(np.arange(L, dtype=np.int32) % 2)                       # L / 2 segments of one slot: the stride over the table
    rows.append(1 - np.arange(L, dtype=np.int32) % 2)                   # ceil(L / 2) of them, the first at 0
    rows.append(np.zeros(L, np.int32))                                  # nothing masked
    odd = segments_mask(L, [(2, min(9, L - 2))])
    odd[0], odd[-1] = 2, -1                                             # neither 2 nor -1 is masked
    rows.append(odd)
    return rows


def batch_masks(g, B, L):
    rows = seam_masks(L)
    out = np.zeros((B, L), np.int32)
    for b in range(B):
        if B == 1:
            out[b] = rows[0]
        elif b < len(rows) and (B > 2 or b == 0):
            out[b] = rows[b]
        elif B == 2:
            out[b] = rows[2 + int(g.integers(0, len(rows) - 2))]
        else:                                                           # random runs
            m = (g.random(L) < 0.75).astype(np.int32)
            m[g.random(L) < 0.05] = (2, -1, 0)[b % 3]
            out[b] = m
    return out


# ------------------------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("L,B", [(64, 1), (64, 65), (130, 2), (130, 65), (1024, 2), (1024, 1), (4096, 1), (4096, 2)])
def test_whole_notes_against_the_restatement(L, B):
    g = np.random.default_rng(L * 100 + B)
    rows = seam_masks(L)
    masks = [batch_masks(g, B, L)]
    if B <= 2:                                                          # every seam mask, B rows at a time
        masks = [np.stack([rows[(i + b) % len(rows)] for b in range(B)]) for i in range(0, len(rows), B)]
    ptok = np.zeros((B, L), np.int32)
    seen = set()
    for n, pmask in enumerate(masks):
        for source in ("int", "pad", "own"):
            if source == "own" and n % 3:
                continue
            cs, ci = own_tables(g, B, L) if source == "own" else int_tables(g, B, L, pad_bias=40 if source == "pad" else 0)
            got = check(cs, ci, ptok, pmask, what="L=%d B=%d mask %d %s" % (L, B, n, source))
            assert (got["status"] == rr.OK).all()
            assert np.array_equal(got["counts"][:, 0], (pmask == 1).sum(1))
            assert np.array_equal(4 * got["counts"][:, 1] + got["counts"][:, 2], got["counts"][:, 0])
            seen.update(got["counts"][:, 3].tolist())
    assert 0 in seen and (L + 1) // 2 in seen and 1 in seen             # no segment, the fullest table, the whole row


def test_two_segments_one_slot_apart_do_not_share_a_decision():
    """adjacent bars: a kept BAR between two regions.  Every pair of lengths around the gap, the gap at every offset inside a 64-bit
    word and across it, with scores that make one side all notes and the other all pads"""
    g = np.random.default_rng(5)
    L = 192
    masks, want_notes = [], []
    for gap in (3, 4, 31, 32, 63, 64, 65, 127, 128):
        for n1, n2 in ((1, 1), (3, 4), (4, 3), (8, 8)):
            if gap - n1 < 0 or gap + 1 + n2 > L:
                continue
            masks.append(segments_mask(L, [(gap - n1, n1), (gap + 1, n2)]))
            want_notes.append(n2 // 4)
    B = len(masks)
    pmask = np.stack(masks)
    cs, ci = int_tables(g, B, L)
    for b in range(B):                                                  # left of the gap pads win every arrival, right of it notes do
        gap = int(np.flatnonzero(pmask[b])[np.flatnonzero(np.diff(np.flatnonzero(pmask[b])) > 1)[0]]) + 1
        cs[b, :gap, rr.PAD], cs[b, gap:, rr.PAD] = 500, -500
    got = check(cs, ci, np.zeros((B, L), np.int32), pmask, what="one slot apart")
    assert (got["status"] == rr.OK).all() and (got["counts"][:, 3] == 2).all()
    assert got["counts"][:, 1].tolist() == want_notes


# ------------------------------------------------------------------------------------------------------------------ availability, -inf, NaN
def test_classes_without_a_token_and_minus_infinity():
    g = np.random.default_rng(6)
    L = 130
    mult4 = segments_mask(L, [(0, 4), (5, 8), (14, 64), (79, 40), (126, 4)])
    not4 = segments_mask(L, [(0, 4), (5, 8), (14, 63), (79, 40)])
    pmask = np.stack([mult4, not4, mult4, mult4, mult4, mult4, not4, mult4])
    B = len(pmask)
    cs, ci = int_tables(g, B, L, pad_bias=20)
    ci[0, :, rr.PAD] = ci[1, :, rr.PAD] = -1                            # no PAD: all notes where every length is a multiple of 4, else no room
    for b, c in zip((2, 3, 4, 5), rr.QUAD):
        ci[b, :, c] = -1                                                # one quad class without a token: all pads
    ci[6, 14 + 62, rr.PAD] = -1                                         # the 63-slot segment cannot end: its last slot has no PAD and 63 is no multiple of 4
    ci[7, :, [rr.EOS, rr.BAR]] = -1                                     # classes a region never reads
    got = check(cs, ci, np.zeros((B, L), np.int32), pmask, what="availability")
    assert got["status"].tolist() == [rr.OK, rr.NO_ROOM, rr.OK, rr.OK, rr.OK, rr.OK, rr.OK, rr.OK]
    assert tuple(got["counts"][0]) == (120, 30, 0, 5) and not got["counts"][1].any() and np.array_equal(got["tokens"][1], ci[1, :, rr.ANY])
    for b in (2, 3, 4, 5):
        assert tuple(got["counts"][b]) == (120, 0, 120, 5)
    assert got["counts"][6, 0] == 115 and got["counts"][6, 2] % 4 == 3   # the 63: notes up to slot 60, then pads, the last slot the DURATION of a note
    # -inf: one class at every position, every class at one position, everything
    cs, ci = int_tables(g, 9, L)
    for b, c in enumerate(rr.USED):
        cs[b, :, c] = -np.inf
    cs[5, 40, :] = -np.inf
    cs[6, :, :] = -np.inf
    cs[7, 14:78, rr.PAD] = -np.inf
    cs[8, 20, rr.PITCH] = -np.inf
    got = check(cs, ci, np.zeros((9, L), np.int32), np.stack([mult4] * 9), what="-inf")
    assert (got["status"] == rr.OK).all() and np.isneginf(got["path_score"][5:7]).all() and np.isfinite(got["path_score"][7:]).all()


def test_nan_and_plus_infinity_under_the_mask_and_outside_it():
    g = np.random.default_rng(7)
    L = 300
    pmask = np.stack([segments_mask(L, [(10, 70), (100, 157), (258, 30)])] * 2)
    cs, ci = int_tables(g, 2, L)
    ptok = np.zeros((2, L), np.int32)
    for bad in (np.nan, np.inf):
        for pos, slot, st in ((10, rr.PAD, rr.NONFINITE), (79, rr.POSITION, rr.NONFINITE), (256, rr.PITCH, rr.NONFINITE), (287, rr.DURATION, rr.NONFINITE),
                              (150, rr.VELOCITY, rr.NONFINITE), (9, rr.PAD, rr.OK), (80, rr.PITCH, rr.OK), (257, rr.DURATION, rr.OK), (299, rr.PAD, rr.OK),
                              (150, rr.EOS, rr.OK), (150, rr.BAR, rr.OK), (150, rr.ANY, rr.OK)):
            hot = cs.copy()
            hot[1, pos, slot] = bad
            got = check(hot, ci, ptok, pmask, what="nonfinite %r at %d slot %d" % (bad, pos, slot))
            assert got["status"].tolist() == [rr.OK, st]
            if st != rr.OK:
                assert np.array_equal(got["tokens"][1], ci[1, :, rr.ANY]) and not got["counts"][1].any() and got["path_score"][1] == 0


# ------------------------------------------------------------------------------------------------------------------ statuses, repeats
def status_batch(g, L=200):
    kinds = ["ok", "not_planned", "ok", "nonfinite", "no_room", "ok", "not_planned_4", "empty", "nonfinite_and_no_room", "ok"]
    B = len(kinds)
    cs, ci = int_tables(g, B, L)
    pmask = np.stack([segments_mask(L, [(5, 40), (46, 4), (60, 100), (170, 29)])] * B)
    pstat = np.zeros(B, np.int32)
    for b, k in enumerate(kinds):
        if k == "not_planned":
            pstat[b] = 1
        elif k == "not_planned_4":
            pstat[b] = 4
            cs[b, 20, rr.PAD] = np.nan                                  # NOT_PLANNED comes first
        elif k == "nonfinite":
            cs[b, 61, rr.PITCH] = np.inf
        elif k in ("no_room", "nonfinite_and_no_room"):
            ci[b, 170:, rr.PAD] = -1                                    # 29 slots without PAD
            if k != "no_room":
                cs[b, 7, rr.VELOCITY] = np.nan
        elif k == "empty":
            pmask[b] = 0
    want = {"ok": rr.OK, "empty": rr.OK, "not_planned": rr.NOT_PLANNED, "not_planned_4": rr.NOT_PLANNED, "nonfinite": rr.NONFINITE,
            "no_room": rr.NO_ROOM, "nonfinite_and_no_room": rr.NONFINITE}
    return cs, ci, pmask, pstat, np.array([want[k] for k in kinds], np.int32)


def test_every_status_inside_one_batch_and_repeated_bits():
    g = np.random.default_rng(8)
    cs, ci, pmask, pstat, want = status_batch(g)
    B, L = pmask.shape
    ptok = np.zeros((B, L), np.int32)
    first = check(cs, ci, ptok, pmask, pstat, what="statuses")
    assert np.array_equal(first["status"], want)
    bad = first["status"] != rr.OK
    assert np.array_equal(first["tokens"][bad], ci[bad][:, :, rr.ANY]) and not first["counts"][bad].any() and not first["path_score"][bad].any()
    assert tuple(first["counts"][7]) == (0, 0, 0, 0) and first["status"][7] == rr.OK
    same(run_regions(cs, ci, ptok, pmask, pstat), first, "repeat")
    # field mode in the same batch: a hostile token under the mask is BAD_PLAN, before NONFINITE and NO_ROOM
    ptok[:, :] = np.array([432, 131, 3, 304], np.int32)[np.arange(L) % 4]
    ptok[2, 61], ptok[3, 100], ptok[4, 10], ptok[9, 198] = 2, 0, 600, -5
    got = check(cs, ci, ptok, pmask, pstat, fields=5, what="field statuses")
    assert got["status"].tolist() == [rr.OK, rr.NOT_PLANNED, rr.BAD_PLAN, rr.BAD_PLAN, rr.BAD_PLAN, rr.OK, rr.NOT_PLANNED, rr.OK, rr.NONFINITE, rr.BAD_PLAN]
    ptok[4, 10] = 434                                                   # position 10 reads POSITION; the duration slots 173, 177, ... still lack nothing
    assert check(cs, ci, ptok, pmask, pstat, fields=5)["status"][4] == rr.OK
    ci[4, 174, rr.PITCH] = -1                                           # 174 % 4 == 2: a pitch slot
    assert check(cs, ci, ptok, pmask, pstat, fields=5)["status"][4] == rr.NO_ROOM


# ------------------------------------------------------------------------------------------------------------------ real plans
def planned(g, B, L, room, fields):
    tokens, pmask, lo, hi = random_batch(g, B, L)
    return device_plan(tokens, pmask, lo, hi, room, fields)


@pytest.mark.parametrize("fields", list(range(1, 15)))
def test_every_field_selection_on_planned_rows(fields):
    g = np.random.default_rng(100 + fields)
    B, L = 12, 130
    p = planned(g, B, L, 0, fields)
    cs, ci = own_tables(g, B, L) if fields % 2 else int_tables(g, B, L)
    got = check(cs, ci, p["tokens"], p["mask"], p["status"], fields, what="fields %d" % fields)
    assert np.array_equal(got["status"] != rr.OK, p["status"] != ir.OK) and (p["status"] == ir.OK).sum() >= 3
    assert not got["counts"][:, 1:3].any() and np.array_equal(got["counts"][:, 0], p["info"][:, 2])
    out, counts = device_splice(got["tokens"], p, fields)
    ok = got["status"] == rr.OK
    assert not counts[ok, 2].any() and np.array_equal(counts[ok, 0], p["info"][ok, 2])   # nothing rejected: every selected slot taken
    # the plain argmax of the same tables is rejected somewhere, so the comparison is not vacuous
    ci_h = ci.cpu().numpy() if isinstance(ci, torch.Tensor) else ci
    assert device_splice(ci_h[:, :, rr.ANY], p, fields)[1][ok, 2].sum() > 0


@pytest.mark.parametrize("room", [0, 2])
@pytest.mark.parametrize("L,B", [(130, 12), (1024, 3)])
def test_real_plans_then_the_splice_drops_nothing_but_pads(L, B, room):
    g = np.random.default_rng(L + room)
    p = planned(g, B, L, room, 15)
    for cs, ci in (own_tables(g, B, L), int_tables(g, B, L, pad_bias=30)):
        got = check(cs, ci, p["tokens"], p["mask"], p["status"], what="plans L=%d room %d" % (L, room))
        assert np.array_equal(got["status"] == rr.NOT_PLANNED, p["status"] != ir.OK) and (got["status"] == rr.OK).any()
        out, counts = device_splice(got["tokens"], p)
        ok = got["status"] == rr.OK
        assert not counts[ok, 2].any()                                  # other == 0
        assert np.array_equal(counts[ok, 0], 4 * got["counts"][ok, 1]) and np.array_equal(counts[ok, 1], got["counts"][ok, 2])
        want_out, want_counts = ir.splice_rows(got["tokens"], p["tokens"], p["mask"], p["status"])
        assert np.array_equal(out, want_out) and np.array_equal(counts, want_counts)
        ci_h = ci.cpu().numpy() if isinstance(ci, torch.Tensor) else ci
        assert device_splice(ci_h[:, :, rr.ANY], p)[1][ok, 2].sum() > 0   # the plain argmax of the same tables loses tokens


# ------------------------------------------------------------------------------------------------------------------ the Python front
@pytest.mark.parametrize("mode", [1, 2])
def test_python_front_is_one_launch_whatever_the_batch(mode):
    g = np.random.default_rng(9)
    V, E, L = 729, 16, 96
    W = torch.nn.Parameter(f32(0.5 * g.standard_normal((V, E))), requires_grad=False)
    norms = ops.row_sqnorm(W)
    model = SimpleNamespace(logits_mode=mode, lm_head=SimpleNamespace(weight=W, bias=f32(np.zeros(V))), word_embedding=SimpleNamespace(weight=W),
                            embedding_norms=lambda: norms)
    for B in (2, 64):
        pmask = np.stack([segments_mask(L, [(20, 12), (33, 9), (50, 40)])] * B)
        pstat = np.zeros(B, np.int32)
        pstat[1] = 2
        plan = SimpleNamespace(tokens=i32(np.zeros((B, L))), mask=i32(pmask), status=i32(pstat), fields=15)
        x = f32(g.standard_normal((B, L, E)))
        cs, ci = gu.class_tables(model, x)
        box = []
        assert library_launches(lambda: box.append(gu.constrain_regions(cs, ci, plan)), strip="()") == ["constrain_regions_kernel"]
        seen = library_launches(lambda: box.append(gu.constrain_region_tokens(model, x, plan)), strip="()")
        assert seen == ["class_argmax_kernel<%d>" % mode, "constrain_regions_kernel"], seen
        (t32, r1), (t64, r2) = box
        assert t32.dtype == torch.int32 and t64.dtype == torch.int64 and t64.shape == (B, L) and torch.equal(t32.long(), t64)
        assert r2.status.shape == (B,) and r2.path_score.shape == (B,) and r2.counts.shape == (B, 4) and isinstance(r2, gu.RegionResult)
        want = rr.constrain_rows(cs.cpu().numpy(), ci.cpu().numpy(), np.zeros((B, L), np.int32), pmask, pstat)
        same(dict(tokens=t32.cpu().numpy(), status=r1.status.cpu().numpy(), path_score=r1.path_score.cpu().numpy(), counts=r1.counts.cpu().numpy()),
             want, "front")
        s = r2.summary()
        assert s["rows"] == {"ok": B - 1, "not_planned": 1, "bad_plan": 0, "nonfinite": 0, "no_room": 0}
        assert s["masked"] == 61 * (B - 1) and s["segments"] == 3 * (B - 1) and 4 * s["notes"] + s["pads"] == s["masked"]
        assert torch.equal(t64[1], ci[1, :, 7].long())
    with pytest.raises(ValueError):
        gu.constrain_regions(cs[:1], ci, plan)
    with pytest.raises(ValueError):
        gu.constrain_regions(cs, ci, SimpleNamespace(tokens=plan.tokens, mask=plan.mask, status=plan.status, fields=0))


def test_refusals():
    src, dst = (torch.zeros(8 * 8, dtype=torch.int32, device=DEV) for _ in range(2))
    a, o = src.data_ptr(), dst.data_ptr()
    lib = _lib.lib()
    ok = dict(score=a, idx=a, ptok=a, pmask=a, pstat=a, fields=15, tokens=o, status=o + 64, path=o + 128, counts=o + 192, B=1, L=8)
    assert lib.mhr_constrain_regions(*ok.values(), None) == 0
    torch.cuda.synchronize()
    for change in (dict(L=4097), dict(L=0), dict(B=0), dict(fields=0), dict(fields=16), dict(score=None), dict(pstat=None), dict(counts=None)):
        assert lib.mhr_constrain_regions(*{**ok, **change}.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"constrain_regions" in lib.mh_last_error()
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.int32)  # noqa: E731
    with pytest.raises(ValueError):
        gu.constrain_regions(torch.zeros(1, 4097, 8, device=DEV), z(1, 4097, 8), SimpleNamespace(tokens=z(1, 4097), mask=z(1, 4097), status=z(1), fields=15))
