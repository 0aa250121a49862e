"""GPU: mhi_infill_plan / mhi_infill_splice (csrc/infill.hip) through the C ABI, bit for bit against the plain-Python restatement
(tests/infill_ref.py).  Every output buffer is sentinel-filled with a guard band on both sides.  Row lengths 64, 255, 256, 257, 1024,
4096 (one chunk of 256 threads, one short of it, one over, many) with 1, 2 and 65 rows whose ranges differ; a BAR, the EOS and a quad
on the seams between threads' chunks and between waves; every status; hostile ranges; room that fits exactly and one slot over; field
masks on malformed quads; the splice on pads, strays, negatives and half quads with junk in every anchored slot."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import infill_ref as ir  # noqa: E402
from gpu_helpers import Guarded, library_launches  # noqa: E402
from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd.utils import infill_util as iu  # noqa: E402
from test_infill_cpu import _hostile_fill  # noqa: E402

DEV = "cuda"
BAR, EOS = ir.BAR, ir.EOS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def plan(tokens, pmask, lo, hi, room=0, fields=15):
    """mhi_infill_plan through the C ABI -> dict of numpy arrays, as infill_ref.plan_rows"""
    B, L = tokens.shape
    t, m, a, b = dev(tokens), dev(pmask), dev(lo), dev(hi)
    out = dict(tokens=Guarded(B, L), mask=Guarded(B, L), status=Guarded(B), info=Guarded(B, 4))
    _lib.check(_lib.lib().mhi_infill_plan(t.data_ptr(), m.data_ptr(), a.data_ptr(), b.data_ptr(), room, fields, out["tokens"].ptr,
                                          out["mask"].ptr, out["status"].ptr, out["info"].ptr, B, L, _lib.current_stream()), "mhi_infill_plan")
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}


def splice(sampled, p, fields=15, status=None):
    B, L = p["tokens"].shape
    s, t, m, st = dev(sampled), dev(p["tokens"]), dev(p["mask"]), dev(p["status"] if status is None else status)
    out, counts = Guarded(B, L), Guarded(B, 4)
    _lib.check(_lib.lib().mhi_infill_splice(s.data_ptr(), t.data_ptr(), m.data_ptr(), st.data_ptr(), fields, out.ptr, counts.ptr, B, L,
                                            _lib.current_stream()), "mhi_infill_splice")
    torch.cuda.synchronize()
    return out.get(), counts.get()


def same_plan(got, want, what=""):
    for k in ("status", "info", "tokens", "mask"):
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


def quad(g):
    return [int(g.integers(432, 560)), int(g.integers(131, 195)), int(g.integers(3, 131)), int(g.integers(304, 432))]


def random_row(g, L, kind="ok", malformed=0.15):
    """-> (tokens [L], prefix mask [L], number of bars): prefix, [tokens before the first BAR,] bars of quads (some broken), EOS, tail"""
    m = int(g.integers(1, max(2, min(20, L // 4))))
    e = int(g.integers(m + 1, L)) if kind != "eos_last" else L - 1
    body = quad(g) if g.random() < 0.3 else []
    while len(body) < e - m:
        body.append(BAR)
        for _ in range(int(g.integers(0, 4))):
            q = quad(g)
            if g.random() < malformed:                            # a broken quad: one token lost, replaced or doubled
                at = int(g.integers(0, 4))
                q = [q[:at] + q[at + 1:], q[:at] + [int(g.choice([0, 200, 600, -3, 729, q[(at + 1) % 4]]))] + q[at + 1:], q[:at] + [q[at]] + q[at:]][int(g.integers(0, 3))]
            body += q
    body = [t if t != EOS else 5 for t in body[:e - m]]
    tail = [int(t) for t in g.choice([0, 0, 0, 7, BAR, EOS, 440, -1], size=L - e - 1)]
    row = [int(t) for t in g.integers(560, 729, size=m)] + body + [EOS] + tail
    mask = [0] * m + [1] * (L - m)
    if kind == "no_eos":
        row = [t if t != EOS else 9 for t in row]
    elif kind == "bad_mask":
        mask = [[1] * L, [0] * L, mask[:-1] + [0], mask[:m] + [2] + mask[m + 1:], [1] + mask[1:] if m > 1 else [0] * L][int(g.integers(0, 5))]
    assert len(row) == L and len(mask) == L
    return row, mask, sum(1 for t in body if t == BAR)


def random_batch(g, B, L, kinds=("ok",) * 6 + ("no_eos", "bad_mask", "bad_range", "eos_last")):
    tokens, pmask, lo, hi = np.zeros((B, L), np.int32), np.zeros((B, L), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        kind = kinds[int(g.integers(0, len(kinds)))] if B > 1 else "ok"
        tokens[b], pmask[b], nb = random_row(g, L, kind)
        if kind == "bad_range" or nb == 0:
            lo[b], hi[b] = [(-1, 1), (0, nb + 1), (1, 1), (nb, nb + 1), (2, 1), (-2 ** 31, 2 ** 31 - 1)][int(g.integers(0, 6))]
        else:
            lo[b] = int(g.integers(0, nb))
            hi[b] = int(g.integers(lo[b] + 1, nb + 1))
    return tokens, pmask, lo, hi


def hostile_sample(g, p):
    """junk in every anchored slot, hostile tokens in the region"""
    B, L = p["tokens"].shape
    s = g.integers(-5, 800, size=(B, L)).astype(np.int32)
    for b in range(B):
        region = np.flatnonzero(p["mask"][b])
        s[b, region] = _hostile_fill(g, len(region)).astype(np.int64).astype(np.int32)
    return s


# ------------------------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("L", [64, 255, 256, 257, 1024, 4096])
def test_plan_and_splice_match_the_restatement(L, B):
    g = np.random.default_rng(1000 * L + B)
    tokens, pmask, lo, hi = random_batch(g, B, L)
    seen = set()
    for room, fields in ((int(g.integers(0, 3)), 15), (0, int(g.integers(1, 15)))):
        got = plan(tokens, pmask, lo, hi, room, fields)
        want = ir.plan_rows(tokens, pmask, lo, hi, room, fields)
        same_plan(got, want, (room, fields))
        seen |= set(got["status"].tolist())
        sampled = hostile_sample(g, got)
        out, counts = splice(sampled, got, fields)
        wout, wcounts = ir.splice_rows(sampled, want["tokens"], want["mask"], want["status"], fields)
        assert np.array_equal(counts, wcounts) and np.array_equal(out, wout), (room, fields)
        ok = got["status"] == ir.OK
        assert np.array_equal(out[~ok], tokens[~ok]) and not counts[~ok].any(), "a row that was not planned comes back unchanged"
        anchored = ok[:, None] & (got["mask"] == 0)
        if fields != 15:
            assert np.array_equal(out[anchored], tokens[anchored])
        else:
            assert (counts[:, 0] % 4 == 0).all() and np.array_equal(counts[:, :3].sum(1), got["info"][:, 2]) and not counts[:, 3].any()
    if B == 65:
        assert {ir.OK, ir.NO_EOS, ir.BAD_MASK, ir.BAD_RANGE} <= seen, seen


def test_rows_longer_than_the_block_can_stage_are_refused():
    L = _lib.lib().mh_batch_max_row() + 1
    assert L == 4097
    t = torch.zeros(1, L, device=DEV, dtype=torch.int32)
    one = torch.zeros(4, device=DEV, dtype=torch.int32)
    rc = _lib.lib().mhi_infill_plan(t.data_ptr(), t.data_ptr(), one.data_ptr(), one.data_ptr(), 0, 15, t.data_ptr(), t.data_ptr(), one.data_ptr(),
                                    one.data_ptr(), 1, L, _lib.current_stream())
    assert rc == _lib.MH_ERR_INVALID and b"4096" in _lib.lib().mh_last_error()
    rc = _lib.lib().mhi_infill_splice(t.data_ptr(), t.data_ptr(), t.data_ptr(), one.data_ptr(), 15, t.data_ptr(), one.data_ptr(), 1, L,
                                      _lib.current_stream())
    assert rc == _lib.MH_ERR_INVALID and b"4096" in _lib.lib().mh_last_error()
    with pytest.raises(_lib.MuseHipError):
        iu.plan_infill(t, t, (0, 1))


# ------------------------------------------------------------------------------------------------------------------ plan cases
def seam_row(g, L, seam, what):
    """a row whose `what` (a BAR, the EOS, or a quad's second token) sits at index `seam`, so that the quad or the bar straddles
    seam - 1 | seam"""
    body = [BAR] + quad(g) + [BAR] + quad(g) + quad(g) + [BAR] + quad(g) + quad(g) + [BAR] + quad(g)
    at = {"bar": 5, "bar_left": 6, "quad": 7, "quad3": 9, "eos": len(body), "eos_left": len(body) + 1}[what]
    m = seam - at                                                  # body[at] lands on index seam (bar_left / eos_left: on seam - 1)
    row = [600] * m + body + [EOS] + [0] * (L - m - len(body) - 1)
    return row, [0] * m + [1] * (L - m)


def test_plan_on_the_seams_between_chunks_and_waves():
    g = np.random.default_rng(7)
    L = 1024
    cases = [(seam, what) for seam in (64, 128, 256, 512) for what in ("bar", "bar_left", "quad", "quad3", "eos", "eos_left")]
    rows = [seam_row(g, L, s, w) for s, w in cases]
    tokens, pmask = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)
    for s, w in ((64, "bar"), (256, "bar_left"), (256, "eos"), (64, "eos_left")):
        t = tokens[cases.index((s, w))]
        assert t[s - (w.endswith("left"))] == (EOS if "eos" in w else BAR)
    i = cases.index((256, "quad"))
    assert [ir.token_class(t) for t in tokens[i, 255:259]] == [0, 1, 2, 3]
    i = cases.index((64, "quad3"))
    assert [ir.token_class(t) for t in tokens[i, 61:65]] == [0, 1, 2, 3]
    B = len(cases)
    for lo, hi in ((0, 4), (1, 2), (1, 3), (3, 4)):
        lo_, hi_ = np.full(B, lo, np.int32), np.full(B, hi, np.int32)
        for room, fields in ((0, 15), (2, 15), (0, 1), (0, 2), (0, 4), (0, 8), (0, 5), (0, 14)):
            got = plan(tokens, pmask, lo_, hi_, room, fields)
            same_plan(got, ir.plan_rows(tokens, pmask, lo_, hi_, room, fields), (lo, hi, room, fields))
            assert not got["status"].any()
            selected = sum([4, 8, 8, 4][lo:hi])                  # the bars hold one, two, two and one quad
            assert (got["info"][:, 2] == selected * bin(fields).count("1") // 4 + got["info"][:, 3]).all()
            assert (got["info"][:, 3] == 4 * room * (hi - lo)).all()


def test_plan_edges_of_the_grammar():
    g = np.random.default_rng(11)
    q = [quad(g) for _ in range(6)]
    P = [600, 601, 602]
    L = 64
    pad = lambda row: row + [0] * (L - len(row))  # noqa: E731
    rows = {
        "empty_bar": pad(P + [BAR, BAR] + q[0] + [BAR, BAR, EOS]),
        "last_bar_ends_at_eos": pad(P + [BAR] + q[0] + [BAR] + q[1] + q[2] + [EOS]),
        "before_first_bar": pad(P + q[0] + q[1][:2] + [BAR] + q[2] + [BAR] + q[3] + [EOS]),
        "eos_at_L_minus_1": P + ([BAR] + q[0] + q[1] + q[2]) * 4 + [BAR] + q[3] + q[4][:3] + [EOS],
        "exact_fit": pad(P + [BAR] + q[0] + [BAR] + q[1] + [EOS])[:3 + 11 + 8],          # e = 13, L = 22: e + 1 + 8 == L
        "one_over": pad(P + [BAR] + q[0] + [BAR] + q[1] + [EOS])[:3 + 11 + 7],
        "cut_by_bar_end": pad(P + [BAR] + q[0][:3] + [BAR] + q[0][3:] + q[1] + [EOS]),
    }
    assert len(rows["eos_at_L_minus_1"]) == 64 and rows["eos_at_L_minus_1"][63] == EOS
    def check(name, lo, hi, room=0, fields=15):
        """one row through the kernel, compared with the restatement -> the kernel's row"""
        row = rows[name]
        pmask = [0] * 3 + [1] * (len(row) - 3)
        got = plan(np.array([row], np.int32), np.array([pmask], np.int32), np.array([lo], np.int32), np.array([hi], np.int32), room, fields)
        got = {k: v[0] for k, v in got.items()}
        want = ir.plan_row(row, pmask, lo, hi, room, fields)
        assert (got["tokens"].tolist(), got["mask"].tolist(), int(got["status"]), tuple(got["info"].tolist())) == want, (name, lo, hi, room, fields)
        return got

    r = check("empty_bar", 0, 1, room=1)
    assert r["info"].tolist() == [4, 8, 4, 4] and r["mask"][4:8].all() and r["tokens"][3:9].tolist() == [BAR, 0, 0, 0, 0, BAR]
    assert check("empty_bar", 0, 1)["info"].tolist() == [4, 4, 0, 0]
    assert check("empty_bar", 2, 4, room=2)["info"].tolist() == [10, 27, 16, 16]
    r = check("last_bar_ends_at_eos", 1, 2, room=1)
    assert r["tokens"][21] == EOS and r["mask"][9:21].all() and not r["mask"][21:].any()
    r = check("before_first_bar", 0, 1)
    assert not r["mask"][:10].any() and r["mask"][10:14].all()
    for lo, hi in ((0, 5), (4, 5), (0, 1)):
        assert check("eos_at_L_minus_1", lo, hi)["status"] == ir.OK
    assert check("eos_at_L_minus_1", 4, 5)["info"].tolist() == [56, 63, 7, 0]
    assert check("eos_at_L_minus_1", 4, 5, room=1)["status"] == ir.OVERFLOW
    assert check("eos_at_L_minus_1", 4, 5, fields=2)["info"].tolist() == [56, 63, 1, 0]      # the three tokens before EOS are no quad
    assert check("exact_fit", 0, 2, room=1)["status"] == ir.OK and check("exact_fit", 0, 2, room=1)["tokens"][21] == EOS
    assert check("one_over", 0, 2, room=1)["status"] == ir.OVERFLOW and check("one_over", 0, 1, room=1)["status"] == ir.OK
    for fields in (1, 2, 4, 8, 5, 14):
        r = check("cut_by_bar_end", 0, 2, fields=fields)
        assert not r["mask"][:9].any() and r["mask"].sum() == bin(fields).count("1")      # only q[1] is whole and inside one bar
    # every status, and the hostile ranges
    assert check("empty_bar", 0, 4, room=100)["status"] == ir.OVERFLOW
    for lo, hi in ((-1, 1), (0, 5), (2, 2), (3, 1), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31), (4, 5)):
        r = check("empty_bar", lo, hi, room=3)
        assert r["status"] == ir.BAD_RANGE and r["tokens"].tolist() == rows["empty_bar"] and not r["mask"].any() and not r["info"].any()
    huge = plan(np.array([rows["empty_bar"]], np.int32), np.array([[0] * 3 + [1] * (L - 3)], np.int32), np.array([0], np.int32),
                np.array([4], np.int32), 2 ** 29)
    assert huge["status"][0] == ir.OVERFLOW                           # 4 room (hi - lo) does not wrap


@pytest.mark.parametrize("fields", [1, 2, 4, 8, 5, 14])
def test_field_masks_on_malformed_quads(fields):
    g = np.random.default_rng(50 + fields)
    B, L = 16, 300
    rows = [random_row(g, L, "ok", malformed=0.5) for _ in range(B)]
    tokens, pmask = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)
    nb = np.array([max(r[2], 1) for r in rows], np.int32)
    lo = np.zeros(B, np.int32)
    got = plan(tokens, pmask, lo, nb, 0, fields)
    want = ir.plan_rows(tokens, pmask, lo, nb, 0, fields)
    same_plan(got, want)
    assert got["mask"].sum() > 0 and np.array_equal(got["tokens"], tokens)
    cls = np.vectorize(ir.token_class)(tokens)
    assert all((fields >> c) & 1 for c in cls[got["mask"] == 1]) and (got["mask"].sum() < (cls >= 0).sum() * bin(fields).count("1") / 4)
    # class mismatches on the way back: every class everywhere
    sampled = g.integers(3, 560, size=(B, L)).astype(np.int32)
    out, counts = splice(sampled, got, fields)
    wout, wcounts = ir.splice_rows(sampled, want["tokens"], want["mask"], want["status"], fields)
    assert np.array_equal(out, wout) and np.array_equal(counts, wcounts)
    assert counts[:, 2].sum() > 0 and counts[:, 0].sum() > 0 and np.array_equal(counts[:, 0] + counts[:, 2], got["info"][:, 2])
    changed = out != tokens
    assert np.array_equal(changed.sum(1), counts[:, 3]) and (got["mask"][changed] == 1).all()
    assert np.array_equal(np.vectorize(ir.token_class)(out), cls)


# ------------------------------------------------------------------------------------------------------------------ splice cases
def test_splice_fills():
    g = np.random.default_rng(23)
    L = 257
    names = ("all_pads", "no_pads", "alternating", "strays", "out_of_vocabulary", "half_quad_at_the_end", "half_quad_at_the_start", "identity")
    rows = []
    while len(rows) < len(names) - 1:
        r = random_row(g, L, "ok", malformed=0.0)
        if r[2] >= 3:
            rows.append(r)
    whole = [600] * 5 + sum(([BAR] + quad(g) + quad(g) + quad(g) for _ in range(4)), []) + [EOS]     # the identity row: whole quads only
    rows.append((whole + [0] * (L - len(whole)), [0] * 5 + [1] * (L - 5), 4))
    tokens, pmask = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)
    B = len(names)
    lo, hi = np.zeros(B, np.int32), np.array([r[2] for r in rows], np.int32)
    for room in (0, 1):
        p = plan(tokens, pmask, lo, hi, room)
        assert not p["status"].any() or room, "without room every row is planned"
        sampled = g.integers(-5, 800, size=(B, L)).astype(np.int32)        # junk in every mask-0 slot
        for b, name in enumerate(names):
            region = np.flatnonzero(p["mask"][b])
            n = len(region)
            quads = np.array([quad(g) for _ in range(n // 4 + 1)], np.int32).reshape(-1)[:n]
            if name == "all_pads":
                fill = np.zeros(n, np.int32)
            elif name == "no_pads":
                fill = quads
            elif name == "alternating":
                fill = np.where(np.arange(n) % 2 == 0, 0, np.repeat(quads, 2)[:n])
            elif name == "strays":
                fill = quads.copy()
                fill[g.choice(n, size=max(1, n // 9), replace=False)] = g.choice([BAR, EOS], size=max(1, n // 9))
            elif name == "out_of_vocabulary":
                fill = quads.copy()
                fill[g.choice(n, size=max(1, n // 9), replace=False)] = g.choice([-1, -2 ** 31, 560, 729, 2 ** 31 - 1, 195], size=max(1, n // 9))
            elif name == "half_quad_at_the_end":                            # each bar's last quad loses its duration
                fill = p["tokens"][b, region].copy()
                fill[np.flatnonzero(np.diff(region, append=L + 9) > 1)] = 0
            elif name == "half_quad_at_the_start":                          # each bar's first quad loses its position
                fill = p["tokens"][b, region].copy()
                fill[np.flatnonzero(np.diff(region, prepend=-9) > 1)] = 0
            else:
                fill = p["tokens"][b, region]
            sampled[b, region] = fill
        out, counts = splice(sampled, p)
        wout, wcounts = ir.splice_rows(sampled, p["tokens"], p["mask"], p["status"])
        assert np.array_equal(out, wout) and np.array_equal(counts, wcounts), room
        ok = p["status"] == ir.OK
        assert (counts[:, 0] % 4 == 0).all() and np.array_equal(counts[:, :3].sum(1), p["info"][:, 2]) and np.array_equal(out[~ok], tokens[~ok])
        by = dict(zip(names, range(B)))
        if room == 0:
            assert counts[by["all_pads"]].tolist() == [0, p["info"][by["all_pads"], 2], 0, 0]
            assert counts[by["no_pads"], 1] == 0 and counts[by["strays"], 2] > 0 and counts[by["out_of_vocabulary"], 2] > 0
            assert counts[by["half_quad_at_the_end"], 2] > 0 and counts[by["half_quad_at_the_start"], 2] > 0
        b = by["identity"]
        assert ok[b] and np.array_equal(out[b], tokens[b]) and counts[b].tolist() == [48, 16 * room, 0, 0], "the plan's own tokens give the piece back"
    # a status other than OK wins over whatever the mask says
    p = plan(tokens, pmask, lo, hi, 0)
    for code in (ir.NO_EOS, ir.BAD_MASK, ir.BAD_RANGE, ir.OVERFLOW, 99, -1):
        out, counts = splice(sampled, p, status=np.full(B, code, np.int32))
        assert np.array_equal(out, p["tokens"]) and not counts.any()


# ------------------------------------------------------------------------------------------------------------------ launches
def test_python_front_repeats_its_bits_and_launches_twice_whatever_the_batch():
    g = np.random.default_rng(3)
    counts = {}
    for B in (2, 64):
        tokens, pmask, lo, hi = random_batch(g, B, 300)
        bars = torch.from_numpy(np.stack([lo, hi], 1))
        want = ir.plan_rows(tokens, pmask, lo, hi, 1)
        first = None
        for rep in range(2):
            p = iu.plan_infill(torch.from_numpy(tokens), torch.from_numpy(pmask), bars.to(DEV) if rep else bars, room=1)
            same_plan(dict(tokens=p.tokens.cpu().numpy(), mask=p.mask.cpu().numpy(), status=p.status.cpu().numpy(), info=p.info.cpu().numpy()), want)
            sampled = torch.from_numpy(hostile_sample(np.random.default_rng(B), want)).to(DEV).long()
            out, cnt = iu.splice_infill(p, sampled)
            assert out.dtype == torch.int32 and cnt.dtype == torch.int32 and p.fields == 15 and p.prefix_mask.dtype == torch.int32
            if first is None:
                first = (out.clone(), cnt.clone())
                wout, wcnt = ir.splice_rows(sampled.cpu().numpy(), want["tokens"], want["mask"], want["status"])
                assert np.array_equal(out.cpu().numpy(), wout) and np.array_equal(cnt.cpu().numpy(), wcnt)
            else:
                assert torch.equal(out, first[0]) and torch.equal(cnt, first[1]), "a repeated call gives the same bits"
        res = iu.InfillResult(p, cnt)
        s = res.summary()
        assert s["rows"] == dict(zip(("ok", "no_eos", "bad_mask", "bad_range", "overflow"), np.bincount(want["status"], minlength=5).tolist()))
        assert [s[k] for k in ("kept", "pads", "other", "changed")] == wcnt.sum(0).tolist()
        ids, mk = torch.from_numpy(tokens).to(DEV), torch.from_numpy(pmask).to(DEV)
        counts[B] = library_launches(lambda: iu.splice_infill(iu.plan_infill(ids, mk, (0, 1), room=1), sampled))
    assert counts[2] == counts[64] and len(counts[2]) == 2, counts
    assert counts[2][0].startswith("infill_plan_kernel") and counts[2][1].startswith("infill_splice_kernel")
