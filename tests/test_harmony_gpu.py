"""GPU: mhh_harmony_counts (csrc/harmony.hip) through the C ABI, bit for bit against the plain-Python restatement
(tests/harmony_ref.py).  Every output buffer is sentinel-filled with a guard band on both sides and every element is compared.  Note
counts around the 256-thread pass (0, 1, 63, 64, 65, 255, 256, 257, the capacity, 32768), chord counts around the same seams up to
4096, each sorted (bisection), with one swapped pair and reversed (linear scan); chords on, one tick before and one tick after note
onsets; all keys and time signatures; hostile pitches, ticks and lengths; every max_bars edge; masks; every status over junk lists;
1, 2 and 65 rows; repeated bits; one launch; every refusal; 512 generated ComMU-shaped pieces through decode_tokens."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import harmony_ref as hr  # noqa: E402
from gpu_helpers import SENTINEL, Guarded, library_launches, same  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402

DEV = "cuda"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def run(notes, chords, counts3, meta, valid=None, max_bars=0, hist=True):
    """mhh_harmony_counts through the C ABI -> dict of numpy arrays, as harmony_ref.batch_counts"""
    B, max_notes, max_chords = notes.shape[0], notes.shape[1], chords.shape[1]
    n, c, k, m = dev(notes), dev(chords), dev(counts3), dev(meta)
    v = None if valid is None else dev(valid)
    out = dict(counts=Guarded(B, 8), status=Guarded(B))
    if hist:
        out["hist"] = Guarded(B, 12)
    if max_bars:
        out["bars"] = Guarded(B, max_bars, 4)
    _lib.check(_lib.lib().mhh_harmony_counts(n.data_ptr(), c.data_ptr(), k.data_ptr(), m.data_ptr(), None if v is None else v.data_ptr(),
                                             out["counts"].ptr, out["hist"].ptr if hist else None, out["bars"].ptr if max_bars else None,
                                             out["status"].ptr, B, max_notes, max_chords, max_bars, _lib.current_stream()), "mhh_harmony_counts")
    torch.cuda.synchronize()
    return {name: g.get() for name, g in out.items()}


def check(notes, chords, counts3, meta, valid=None, max_bars=0, hist=True, what=""):
    got = run(notes, chords, counts3, meta, valid, max_bars, hist)
    want = hr.batch_counts(notes, chords, counts3, meta, valid, max_bars)
    assert set(got) == {"counts", "status"} | ({"hist"} if hist else set()) | ({"bars"} if max_bars else set())
    same(got, want, what)
    return got


def junk(g, *shape):
    return g.integers(I32_MIN, I32_MAX, size=shape, endpoint=True).astype(np.int32)


def fill_row(g, notes, chords, n, c, order="sorted", tpb=1920, bars=6):
    """n notes and c chords into one row of junk-filled lists.  Chord ticks on a grid of 120 (equal ticks are common), tokens mostly
    chords, some NN and strangers; half of the notes start on, one tick before or one tick after a chord, the others anywhere from
    before the first chord to behind the last; hostile pitches, negative starts, ends before starts and lengths above 65535 mixed in."""
    span = bars * tpb
    ticks = np.sort(g.integers(0, span // 120, size=c) * 120)
    tokens = np.where(g.random(c) < 0.85, g.integers(195, 303, size=c), g.choice([303, 304, 194, 0, -1, I32_MAX, I32_MIN], size=c))
    if order == "swapped" and c >= 2 and ticks[0] != ticks[-1]:
        i = int(g.integers(0, c - 1))
        j = i + 1
        while ticks[j] == ticks[i]:                                # c >= 2 and not all equal: wrap around until the ticks differ
            i, j = (i + 1) % (c - 1), (i + 1) % (c - 1) + 1
        ticks[[i, j]], tokens[[i, j]] = ticks[[j, i]], tokens[[j, i]]
    elif order == "reversed":
        ticks, tokens = ticks[::-1], tokens[::-1]
    chords[:c, 0], chords[:c, 1] = ticks, tokens
    start = g.integers(-300, span + tpb, size=n)
    if c:
        seam = g.random(n) < 0.5
        start = np.where(seam, ticks[g.integers(0, c, size=n)] + g.integers(-1, 2, size=n), start)
    length = np.where(g.random(n) < 0.8, g.integers(1, 2000, size=n), g.choice([70000, 65535, 65536, -5, 0, 10 ** 6], size=n))
    pitch = np.where(g.random(n) < 0.85, g.integers(0, 128, size=n), g.choice([-1, 128, I32_MIN, I32_MAX, -12, 255, -13], size=n))
    notes[:n, 0], notes[:n, 1], notes[:n, 2], notes[:n, 3] = start, start + length, pitch, g.integers(0, 128, size=n)


def make(g, ns, cs, max_notes, max_chords, orders=("sorted",), metas=None):
    """one row per entry of ns / cs / orders (cycled to the longest) -> notes, chords, counts3, meta"""
    B = max(len(ns), len(cs), len(orders), len(metas) if metas is not None else 0)
    notes, chords, counts3 = junk(g, B, max_notes, 4), junk(g, B, max_chords, 2), junk(g, B, 3)
    meta = np.tile(np.array(META, np.int32), (B, 1))
    for b in range(B):
        if metas is not None:
            meta[b, 1], meta[b, 2] = metas[b % len(metas)]
        else:
            meta[b, 1], meta[b, 2] = int(g.integers(602, 626)), int(g.integers(627, 631))
        n, c = ns[b % len(ns)], cs[b % len(cs)]
        counts3[b, 0], counts3[b, 1] = n, c
        fill_row(g, notes[b], chords[b], n, c, orders[b % len(orders)], hr.TICKS_PER_BAR[int(meta[b, 2])])
    return notes, chords, counts3, meta


# ------------------------------------------------------------------------------------------------------------------ the matrix
NOTE_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 600]


def test_note_counts_around_the_pass_and_the_capacity():
    g = np.random.default_rng(1)
    args = make(g, NOTE_COUNTS, [7, 5, 3], 600, 16, ("sorted", "reversed"))
    got = check(*args, max_bars=8)
    assert got["counts"][:, 0].tolist() == NOTE_COUNTS and (got["status"] == hr.OK).all()
    assert got["counts"][2:, 1].min() > 0 and got["counts"][2:, 2].min() > 0, "the cases judge something"


def test_the_largest_row_keeps_its_sums_in_int32():
    g = np.random.default_rng(2)
    notes, chords, counts3, meta = make(g, [32768], [3], 32768, 4)
    notes[0, :, 1] = notes[0, :, 0] + 70000                          # every length is cut at 65535
    chords[0, :3, 0] = [0, 0, 1920]
    got = check(notes, chords, counts3, meta, max_bars=3)
    assert got["counts"][0, 0] == 32768 and got["counts"][0, 4] == 32768 * 65535 < 2 ** 31


CHORD_COUNTS = [0, 1, 2, 63, 64, 65, 257, 4096]


@pytest.mark.parametrize("order", ["sorted", "swapped", "reversed"])
def test_chord_counts_on_the_bisection_and_on_the_scan(order):
    g = np.random.default_rng(10 + len(order))
    notes, chords, counts3, meta = make(g, [24], CHORD_COUNTS, 24, 4096, (order,))
    if order != "sorted":
        for b, c in enumerate(CHORD_COUNTS):
            falls = bool((np.diff(chords[b, :c, 0].astype(np.int64)) < 0).any())
            assert falls == (c >= 2), "rows of two and more chords take the scan"
    else:
        assert all((np.diff(chords[b, :c, 0].astype(np.int64)) >= 0).all() for b, c in enumerate(CHORD_COUNTS))
        assert any((np.diff(chords[b, :c, 0]) == 0).any() for b, c in enumerate(CHORD_COUNTS)), "equal ticks on the bisection"
    got = check(notes, chords, counts3, meta, max_bars=7, what=order)
    assert (got["status"] == hr.OK).all() and got["counts"][3:, 1].min() > 0
    # the answer does not depend on the order: the stable sort by tick of every row gives the same bits
    stable = chords.copy()
    for b, c in enumerate(CHORD_COUNTS):
        stable[b, :c] = chords[b, :c][np.argsort(chords[b, :c, 0], kind="stable")]
    same(run(notes, stable, counts3, meta, max_bars=7), got, "stable sort")


def test_a_chord_on_every_seam():
    """chords at a note's start, one tick before and one tick after, sorted and not; c# major against c major tells which is in force:
    the answers are worked out here"""
    c_maj, cs_maj = 195 + du.CHORD_NAMES.index("c"), 195 + du.CHORD_NAMES.index("c#")
    rows = []
    for ticks in ([0, 1000], [0, 999], [0, 1001], [1000, 0], [1001, 0], [999, 0], [1000, 1000], [1001], [1000], [-5, 1000, 1000, 999]):
        toks = [c_maj if i % 2 == 0 else cs_maj for i in range(len(ticks))]
        rows.append(list(zip(ticks, toks)))
    B = len(rows)
    notes, chords, counts3 = np.zeros((B, 2, 4), np.int32), np.zeros((B, 4, 2), np.int32), np.zeros((B, 3), np.int32)
    for b, ch in enumerate(rows):
        notes[b] = [[1000, 1100, 61, 64], [1000, 1100, 65, 64]]       # c# and f: both in c# major, neither in c major
        chords[b, :len(ch)] = ch
        counts3[b] = [2, len(ch), 0]
    got = check(notes, chords, counts3, np.tile(np.array(META, np.int32), (B, 1)))
    # in force: c# at 1000 | c# at 999 | c at 0 | c at 1000 | c# at 0 | c at 999 | the later c# at 1000 | none | c at 1000 | the later c at 1000
    assert got["counts"][:, 1].tolist() == [2, 2, 2, 2, 2, 2, 2, 0, 2, 2]
    assert got["counts"][:, 2].tolist() == [2, 2, 0, 0, 2, 0, 2, 0, 0, 0]


def test_all_keys_and_time_signatures():
    g = np.random.default_rng(4)
    metas = [(k, t) for k in range(602, 626) for t in range(627, 631)]
    args = make(g, [40], [6], 40, 8, ("sorted", "swapped"), metas)
    got = check(*args, max_bars=9)
    assert (got["status"] == hr.OK).all() and len({tuple(r) for r in got["counts"][:, 3:4].tolist()}) > 5


def test_hostile_pitches_ticks_and_lengths():
    c_maj = 195 + du.CHORD_NAMES.index("c")
    rows = [[(0, 100, -1, 1), (0, 100, 128, 1), (0, 100, I32_MIN, 1), (0, 100, I32_MAX, 1), (0, 100, -12, 1)],
            [(-1, 100, 60, 1), (I32_MIN, I32_MAX, 60, 1), (I32_MAX, I32_MIN, 64, 1), (-1920, -1, 67, 1), (I32_MAX, I32_MAX, 60, 1)],
            [(0, 65535, 60, 1), (0, 65536, 60, 1), (5, 4, 60, 1), (7, 7, 60, 1), (0, I32_MAX, 60, 1)]]
    notes = np.array(rows, np.int64).astype(np.int32)
    chords = np.array([[(0, c_maj)], [(I32_MIN, c_maj)], [(0, c_maj)]], np.int64).astype(np.int32)
    counts3 = np.array([[5, 1, 0]] * 3, np.int32)
    got = check(notes, chords, counts3, np.tile(np.array(META, np.int32), (3, 1)), max_bars=4)
    assert got["hist"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1]     # -1 -> 11, 128 -> 8, INT32_MIN -> 4, INT32_MAX -> 7, -12 -> 0
    assert got["counts"][2, 4] == 65535 + 65535 + 0 + 0 + 65535
    assert got["counts"][1, 1] == 5 and got["counts"][1, 7] == 1 + I32_MAX // 1920


@pytest.mark.parametrize("hist", [True, False])
def test_max_bars_edges(hist):
    g = np.random.default_rng(6)
    notes, chords, counts3, meta = make(g, [30, 50, 2], [5], 50, 8, ("sorted", "reversed"), [(602, 627)])
    notes[2, 0], notes[2, 1] = [511 * 1920, 511 * 1920 + 10, 60, 1], [512 * 1920, 512 * 1920 + 10, 64, 1]
    used = hr.batch_counts(notes, chords, counts3, meta)["counts"][:, 7].tolist()
    assert used[2] == 513 and 2 < used[0] < 12
    for max_bars in (0, 1, used[0] - 1, used[0], 512):
        got = check(notes, chords, counts3, meta, max_bars=max_bars, hist=hist, what=max_bars)
        assert got["counts"][:, 7].tolist() == used
        if max_bars >= used[0]:
            assert got["bars"][0].sum(0).tolist() == got["counts"][0, :4].tolist()
        elif max_bars:
            assert got["bars"][0, :, 0].sum() < got["counts"][0, 0]
        if max_bars == 512:
            assert got["bars"][2, 511, 0] == 1 and got["bars"][2, :, 0].sum() == 1 and got["counts"][2, 0] == 2, "bar 512 is in the totals only"


def test_masks_and_every_status_over_junk_lists():
    g = np.random.default_rng(7)
    B = 16
    notes, chords, counts3, meta = make(g, [33] * B, [4], 40, 6)
    for valid in (None, np.array([1] * 5 + [0] + [1] * 10), np.arange(B) % 2, np.zeros(B, np.int32), np.where(np.arange(B) % 2, -7, 0)):
        got = check(notes, chords, counts3, meta, valid, max_bars=8, what=None if valid is None else valid.tolist())
        want = np.zeros(B, np.int32) if valid is None else np.where(np.asarray(valid) != 0, hr.OK, hr.MASKED)
        assert got["status"].tolist() == want.tolist()
    # refused rows: their lists are junk, their counts hostile; every output of theirs is zero
    notes, chords = junk(g, B, 40, 4), junk(g, B, 6, 2)
    fill_row(g, notes[0], chords[0], 33, 4)
    counts3[:, :2] = [[33, 4], [-1, 4], [41, 4], [33, -1], [33, 7], [I32_MIN, 0], [I32_MAX, 0], [0, I32_MAX], [33, 4], [33, 4], [33, 4],
                      [33, 4], [40, 6], [33, 4], [-1, -1], [33, 4]]
    meta[8:12, 1:3] = [[601, 627], [626, 627], [602, 626], [602, 631]]
    meta[13] = junk(g, 11)
    meta[14, 1] = 0                                                  # BAD_META comes before BAD_COUNTS
    valid = np.ones(B, np.int32)
    valid[15] = 0
    meta[15, 1] = 0                                                  # MASKED comes before both
    fill_row(g, notes[12], chords[12], 40, 6)
    got = check(notes, chords, counts3, meta, valid, max_bars=8)
    C_, M_, K_ = hr.BAD_COUNTS, hr.BAD_META, hr.MASKED
    assert got["status"].tolist() == [0, C_, C_, C_, C_, C_, C_, C_, M_, M_, M_, M_, 0, M_, M_, K_]
    refused = got["status"] != hr.OK
    assert not got["counts"][refused].any() and not got["hist"][refused].any() and not got["bars"][refused].any()
    assert got["counts"][0, 0] == 33 and got["counts"][12, 0] == 40


@pytest.mark.parametrize("B", [1, 2, 65])
def test_batch_sizes_and_the_same_bits_on_a_repeated_call(B):
    g = np.random.default_rng(100 + B)
    args = make(g, [int(g.integers(0, 300)) for _ in range(B)], [int(g.integers(0, 40)) for _ in range(B)], 300, 40,
                ("sorted", "swapped", "reversed")[:B])
    assert len(args[0]) == B
    valid = (g.random(B) < 0.8).astype(np.int32)
    first = check(*args, valid, max_bars=8)
    same(run(*args, valid, max_bars=8), first, "repeat")


def test_python_front_launches_once_whatever_the_batch():
    g = np.random.default_rng(9)
    seen = {}
    for B in (2, 64):
        notes, chords, counts3, meta = (dev(a) for a in make(g, [50] * B, [9], 64, 12, ("sorted", "reversed")))
        want = hr.batch_counts(notes.cpu().numpy(), chords.cpu().numpy(), counts3.cpu().numpy(), meta.cpu().numpy(), None, 5)
        box = []
        seen[B] = library_launches(lambda: box.append(metric.harmony_counts_raw(notes, chords, counts3, meta, None, 5, True)))
        hc = box[0]
        assert hc.counts.dtype == torch.int32 and hc.bars.shape == (B, 5, 4) and hc.hist.shape == (B, 12)
        same(dict(counts=hc.counts.cpu().numpy(), status=hc.status.cpu().numpy(), bars=hc.bars.cpu().numpy(), hist=hc.hist.cpu().numpy()), want)
        plain = metric.harmony_counts_raw(notes, chords, counts3, meta)
        assert plain.bars is None and plain.hist is None and torch.equal(plain.counts, hc.counts)
    assert seen[2] == seen[64] and len(seen[2]) == 1 and seen[2][0].startswith("harmony_counts_kernel"), seen


def test_every_refusal_leaves_the_outputs_alone():
    lib = _lib.lib()
    g = np.random.default_rng(11)
    n, c, k, m = (dev(a) for a in make(g, [3], [2], 4, 4))
    v = dev(np.ones(1))
    out, hist, bars, status = Guarded(1, 8), Guarded(1, 12), Guarded(1, 2, 4), Guarded(1)
    ok = dict(notes=n.data_ptr(), chords=c.data_ptr(), counts3=k.data_ptr(), meta=m.data_ptr(), valid=v.data_ptr(), out=out.ptr, hist=hist.ptr,
              bars=bars.ptr, status=status.ptr, B=1, max_notes=4, max_chords=4, max_bars=2)
    bad = [dict(notes=None), dict(chords=None), dict(counts3=None), dict(meta=None), dict(out=None), dict(status=None), dict(B=0), dict(B=-1),
           dict(max_notes=0), dict(max_notes=32769), dict(max_chords=0), dict(max_chords=4097), dict(max_bars=-1), dict(max_bars=513),
           dict(bars=None), dict(max_bars=0)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhh_harmony_counts(*args.values(), _lib.current_stream()) == _lib.MH_ERR_INVALID, change
        assert b"harmony_counts" in lib.mh_last_error()
    torch.cuda.synchronize()
    for buf in (out, hist, bars, status):
        assert (buf.get() == SENTINEL).all(), "a refused call writes nothing"
    for change in (dict(valid=None), dict(hist=None), dict(bars=None, max_bars=0)):     # what may be NULL
        args = {**ok, **change}
        assert lib.mhh_harmony_counts(*args.values(), _lib.current_stream()) == 0, change
    torch.cuda.synchronize()
    assert status.get().tolist() == [hr.OK] and out.get()[0, 0] == 3
    for kw in (dict(max_bars=513), dict(max_bars=-1)):
        with pytest.raises(ValueError):
            metric.harmony_counts_raw(n, c, k, m, **kw)
    with pytest.raises(ValueError):
        metric.harmony_counts_raw(n, c, k[:, :2], m)


def test_512_generated_pieces_through_decode_tokens():
    tokens, masks, kinds = dr.make_batch(23, 320, (dr.BATCH_KINDS * 6)[:512])
    dec = du.decode_tokens(torch.from_numpy(tokens).to(DEV), torch.from_numpy(masks).to(DEV))
    hc = metric.harmony_counts(dec, max_bars=12, return_hist=True)
    status = dec.status.cpu().numpy()
    want = hr.batch_counts(dec.notes.cpu().numpy(), dec.chords.cpu().numpy(), dec.counts.cpu().numpy(), dec.meta.cpu().numpy(),
                           status == dr.OK, 12)
    same(dict(counts=hc.counts.cpu().numpy(), status=hc.status.cpu().numpy(), bars=hc.bars.cpu().numpy(), hist=hc.hist.cpu().numpy()), want)
    ok = want["status"] == hr.OK
    assert ok.sum() > 200 and (want["status"][status != dr.OK] == hr.MASKED).all()
    assert want["counts"][ok, 1].sum() > 3000 and 0 < want["counts"][ok, 2].sum() < want["counts"][ok, 1].sum()
    assert (want["counts"][ok, 7] <= 12).all() and np.array_equal(want["bars"][ok].sum(1), want["counts"][ok, :4])
    total, wrong = metric.Controllability_Harmony(dec)
    assert (total, wrong) == (int(want["counts"][:, 1].sum()), int(want["counts"][:, 1].sum() - want["counts"][:, 2].sum()))
