"""GPU: mhm_structure_counts (csrc/structure.hip) through the C ABI, bit for bit against the plain-Python restatement
(tests/structure_ref.py), the two float64 entropy sums included: both take the same k log2 k table.  Every output buffer is
sentinel-filled with a guard band on both sides and every element is compared.  Note counts around the 256-thread pass (0, 1, 2, 255,
256, 257, the capacity, 32768); bars_used 1, 3, 4, 5, max_bars - 1 and max_bars at max_bars 1, 4, 64 and 512; slot and bar seams of all
four time signatures, skipped notes, hostile ticks and pitches; shuffled notes; 1, 2 and 65 rows; masks; every status over junk lists;
bars NULL and not; repeated bits; one launch; every refusal; 512 generated ComMU-shaped pieces through decode_tokens."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import structure_ref as sr  # noqa: E402
from gpu_helpers import SENTINEL, Guarded, library_launches, same  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402

DEV = "cuda"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]
TABLE = metric.xlog2x_host(32768)            # every call takes a prefix of this one table, the kernel and the restatement alike


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def run(notes, counts3, meta, valid=None, max_bars=8, bars=True):
    """mhm_structure_counts through the C ABI -> dict of numpy arrays, as structure_ref.batch_counts"""
    B, max_notes = notes.shape[0], notes.shape[1]
    n, k, m = dev(notes), dev(counts3), dev(meta)
    v = None if valid is None else dev(valid)
    table = torch.from_numpy(TABLE[:max_notes + 1].copy()).to(DEV)
    out = dict(counts=Guarded(B, 16), entropy=Guarded(B, 2, dtype=torch.float64), status=Guarded(B))
    if bars:
        out["bars"] = Guarded(B, max_bars, 16)
    _lib.check(_lib.lib().mhm_structure_counts(n.data_ptr(), k.data_ptr(), m.data_ptr(), None if v is None else v.data_ptr(), table.data_ptr(),
                                               out["counts"].ptr, out["entropy"].ptr, out["bars"].ptr if bars else None, out["status"].ptr,
                                               B, max_notes, max_bars, _lib.current_stream()), "mhm_structure_counts")
    torch.cuda.synchronize()
    return {name: g.get() for name, g in out.items()}


def check(notes, counts3, meta, valid=None, max_bars=8, bars=True, what=""):
    got = run(notes, counts3, meta, valid, max_bars, bars)
    want = sr.batch_counts(notes, counts3, meta, TABLE, valid, max_bars)
    assert set(got) == {"counts", "entropy", "status"} | ({"bars"} if bars else set())
    same(got, want, what)
    return got


def junk(g, *shape):
    return g.integers(I32_MIN, I32_MAX, size=shape, endpoint=True).astype(np.int32)


def fill_row(g, notes, n, tpb=1920, bars=6):
    """n notes into one row of a junk-filled list: most start inside `bars` bars, on and off the sixteenth-note grid, some before 0 and
    some behind the last bar; pitches mostly 0..127 and clustered so that bars differ in entropy, hostile ones mixed in"""
    span = bars * tpb
    start = np.where(g.random(n) < 0.6, g.integers(0, max(span // 120, 1), size=n) * 120 + g.choice([0, 0, 1, 119], size=n), g.integers(-300, span + tpb, size=n))
    centre = 36 + 12 * ((start // tpb) % 5)
    pitch = np.where(g.random(n) < 0.9, np.clip(centre + g.integers(-7, 8, size=n), 0, 127), g.choice([-1, 128, I32_MIN, I32_MAX, -12, 255, 0, 127], size=n))
    notes[:n, 0], notes[:n, 1], notes[:n, 2], notes[:n, 3] = start, start + g.integers(1, 2000, size=n), pitch, g.integers(0, 128, size=n)


def make(g, ns, max_notes, bars=(6,), metas=None):
    """one row per entry of ns / bars / metas (cycled to the longest) -> notes, counts3, meta"""
    B = max(len(ns), len(bars), len(metas) if metas is not None else 0)
    notes, counts3 = junk(g, B, max_notes, 4), junk(g, B, 3)
    meta = np.tile(np.array(META, np.int32), (B, 1))
    for b in range(B):
        meta[b, 1], meta[b, 2] = metas[b % len(metas)] if metas is not None else (int(g.integers(602, 626)), int(g.integers(627, 631)))
        counts3[b, 0] = ns[b % len(ns)]
        fill_row(g, notes[b], ns[b % len(ns)], sr.TICKS_PER_BAR[int(meta[b, 2])], bars[b % len(bars)])
    return notes, counts3, meta


# ------------------------------------------------------------------------------------------------------------------ the matrix
NOTE_COUNTS = [0, 1, 2, 255, 256, 257, 600]


def test_note_counts_around_the_pass_and_the_capacity():
    g = np.random.default_rng(1)
    args = make(g, NOTE_COUNTS, 600)
    got = check(*args, max_bars=8)
    assert (got["counts"][:, 0] + got["counts"][:, 1]).tolist() == NOTE_COUNTS and (got["status"] == sr.OK).all()
    assert got["counts"][3:, 1].min() > 0 and got["counts"][3:, 13].min() > 0 and got["entropy"][3:].min() > 1.0, "the cases count something"


def test_the_largest_row():
    g = np.random.default_rng(2)
    notes, counts3, meta = make(g, [32768], 32768, bars=(40,), metas=[(602, 630)])
    got = check(notes, counts3, meta, max_bars=48)
    assert got["counts"][0, 0] > 25000 and got["counts"][0, 2] == 41 and got["counts"][0, 11] == 24
    # all of them on one pitch in one slot of one bar: the most contended atomics, the largest histogram entry
    notes[0, :, 0], notes[0, :, 2] = 5 * 2880 + 7, 64
    got = check(notes, counts3, meta, max_bars=6)
    assert got["counts"][0].tolist() == [32768, 0, 6, 1, 1, 1, 64, 64, 1, 15, 5, 24, 1, 1, 0, 0] and not got["entropy"].any()


@pytest.mark.parametrize("max_bars", [1, 4, 64, 512])
def test_bars_used_at_every_table_size(max_bars):
    g = np.random.default_rng(20 + max_bars)
    want_used = sorted({u for u in (1, 3, 4, 5, max_bars - 1, max_bars) if 1 <= u <= max_bars})
    ts = [627, 628, 629, 630]
    B = len(want_used)
    notes, counts3 = junk(g, B, 700, 4), junk(g, B, 3)
    meta = np.tile(np.array(META, np.int32), (B, 1))
    for b, used in enumerate(want_used):
        meta[b, 2] = ts[b % 4]
        tpb = sr.TICKS_PER_BAR[ts[b % 4]]
        n = min(700, 3 * used + 1)
        counts3[b, 0] = n
        fill_row(g, notes[b], n, tpb, used)
        notes[b, :n, 0] = np.clip(notes[b, :n, 0], 0, used * tpb - 1)
        notes[b, 0, 0], notes[b, 0, 2] = (used - 1) * tpb + 5, 60             # a note in the last bar
        notes[b, 1, 0], notes[b, 1, 2] = max_bars * tpb, 61                   # and one just behind the table: skipped
    got = check(notes, counts3, meta, max_bars=max_bars, what=max_bars)
    used = got["counts"][:, 2].tolist()
    assert used == want_used and (got["counts"][:, 1] >= 1).all()
    assert got["counts"][:, 9].tolist() == [u * (u - 1) // 2 for u in used]
    assert all(0 <= w <= max(0, u - 3) for u, w in zip(used, got["counts"][:, 13].tolist())) and (got["counts"][:, 13] > 0).sum() == sum(u >= 4 for u in used)
    if max_bars == 512:
        assert used[-1] == 512 and got["counts"][-1, 9] == 130816 and got["counts"][-1, 10] > 10 ** 5


@pytest.mark.parametrize("ts", [627, 628, 629, 630])
def test_seams_skipped_notes_and_hostile_ticks(ts):
    tpb = sr.TICKS_PER_BAR[ts]
    Q = tpb // 120
    rows = [[(k * tpb + 119, 0, 60, 1), (k * tpb + 120, 0, 61, 1), (k * tpb - 1, 0, 62, 1), (0, 0, 0, 1), (1, 0, 127, 1)] for k in (1, 2, 3)]
    rows.append([(-1, 5, 60, 1), (4 * tpb, 5, 60, 1), (4 * tpb - 1, 5, 60, 1), (0, 5, -1, 1), (0, 5, 128, 1)])
    rows.append([(I32_MIN, I32_MAX, 60, 1), (I32_MAX, I32_MIN, 60, 1), (0, 0, I32_MIN, 1), (0, 0, I32_MAX, 1), (I32_MAX - 1, 0, 127, 1)])
    notes = np.array(rows, np.int64).astype(np.int32)
    B = len(rows)
    meta = np.tile(np.array(META, np.int32), (B, 1))
    meta[:, 2] = ts
    got = check(notes, np.array([[5, I32_MIN, I32_MAX]] * B, np.int32), meta, max_bars=4, what=ts)
    for b, k in enumerate((1, 2, 3)):
        assert got["bars"][b, k, :4].tolist() == [2, 0b11, 60, 61] and got["bars"][b, k - 1, 1] & (1 << (Q - 1))
    assert got["counts"][3, :4].tolist() == [1, 4, 4, 1] and got["bars"][3, 3, :4].tolist() == [1, 1 << (Q - 1), 60, 60]
    assert got["counts"][4].tolist() == [0, 5, 0, 0, 0, 0, -1, -1, 0, 0, 0, Q, 0, 0, 0, 0] and (got["bars"][4, :, 2:4] == -1).all()


def test_the_order_of_the_notes_changes_no_bit():
    g = np.random.default_rng(5)
    notes, counts3, meta = make(g, [600, 257, 31], 600, bars=(7, 3, 12))
    first = check(notes, counts3, meta, max_bars=12)
    for seed in (1, 2, None):                                         # two shuffles, and the list backwards
        shuffled = notes.copy()
        for b in range(3):
            n = int(counts3[b, 0])
            shuffled[b, :n] = notes[b, :n][np.random.default_rng(seed).permutation(n) if seed else np.arange(n)[::-1]]
        assert not np.array_equal(shuffled, notes)
        same(run(shuffled, counts3, meta, max_bars=12), first, "shuffled")


def test_masks_and_every_status_over_junk_lists():
    g = np.random.default_rng(7)
    B = 16
    notes, counts3, meta = make(g, [33] * B, 40)
    for valid in (None, np.array([1] * 5 + [0] + [1] * 10), np.arange(B) % 2, np.zeros(B, np.int32), np.where(np.arange(B) % 2, -7, 0)):
        got = check(notes, counts3, meta, valid, max_bars=8, what=None if valid is None else valid.tolist())
        want = np.zeros(B, np.int32) if valid is None else np.where(np.asarray(valid) != 0, sr.OK, sr.MASKED)
        assert got["status"].tolist() == want.tolist()
    # refused rows: their lists are junk, their counts hostile; every output of theirs is zero
    notes = junk(g, B, 40, 4)
    fill_row(g, notes[0], 33)
    counts3[:, 0] = [33, -1, 41, I32_MIN, I32_MAX, 40, 0, 33, 33, 33, 33, 33, 33, 33, -1, 33]
    meta[:] = np.array(META, np.int32)
    meta[8:12, 1:3] = [[601, 627], [626, 627], [602, 626], [602, 631]]
    meta[13] = junk(g, 11)
    meta[14, 1] = 0                                                  # BAD_META comes before BAD_COUNTS
    valid = np.ones(B, np.int32)
    valid[15] = 0
    meta[15, 1] = 0                                                  # MASKED comes before both
    fill_row(g, notes[5], 40)
    got = check(notes, counts3, meta, valid, max_bars=8)
    C_, M_, K_ = sr.BAD_COUNTS, sr.BAD_META, sr.MASKED
    assert got["status"].tolist() == [0, C_, C_, C_, C_, 0, 0, 0, M_, M_, M_, M_, 0, M_, M_, K_]
    refused = got["status"] != sr.OK
    assert not got["counts"][refused].any() and not got["entropy"][refused].any() and not got["bars"][refused].any()
    assert got["counts"][0, :2].sum() == 33 and got["counts"][5, :2].sum() == 40 and got["counts"][6, :3].tolist() == [0, 0, 0]


@pytest.mark.parametrize("B", [1, 2, 65])
def test_batch_sizes_bars_or_not_and_the_same_bits_on_a_repeated_call(B):
    g = np.random.default_rng(100 + B)
    args = make(g, [int(g.integers(0, 300)) for _ in range(B)], 300, bars=tuple(int(g.integers(1, 12)) for _ in range(B)))
    assert len(args[0]) == B
    valid = (g.random(B) < 0.8).astype(np.int32)
    first = check(*args, valid, max_bars=12)
    same(run(*args, valid, max_bars=12), first, "repeat")
    without = check(*args, valid, max_bars=12, bars=False)
    same(without, first, "bars NULL")


def host(sc):
    out = dict(counts=sc.counts.cpu().numpy(), entropy=sc.entropy.cpu().numpy(), status=sc.status.cpu().numpy())
    if sc.bars is not None:
        out["bars"] = sc.bars.cpu().numpy()
    return out


def test_python_front_launches_once_whatever_the_batch():
    g = np.random.default_rng(9)
    seen = {}
    table = metric.xlog2x_host(64)
    for B in (2, 64):
        arrays = make(g, [50] * B, 64)
        notes, counts3, meta = (dev(a) for a in arrays)
        want = sr.batch_counts(*arrays, table, None, 5)
        metric.xlog2x_table(64, notes.device)                          # the table's upload is cached: not part of a call
        box = []
        seen[B] = library_launches(lambda: box.append(metric.structure_counts_raw(notes, counts3, meta, None, 5, True)))
        sc = box[0]
        assert sc.counts.dtype == torch.int32 and sc.entropy.dtype == torch.float64 and sc.bars.shape == (B, 5, 16) and sc.entropy.shape == (B, 2)
        same(host(sc), want)
        plain = metric.structure_counts_raw(notes, counts3, meta, max_bars=5)
        assert plain.bars is None and torch.equal(plain.counts, sc.counts) and torch.equal(plain.entropy, sc.entropy)
        default = metric.structure_counts_raw(notes, counts3, meta)
        same(host(default), {k: v for k, v in sr.batch_counts(*arrays, table, None, 64).items() if k != "bars"})
    assert seen[2] == seen[64] and len(seen[2]) == 1 and seen[2][0].startswith("structure_counts_kernel"), seen


def test_every_refusal_leaves_the_outputs_alone():
    lib = _lib.lib()
    g = np.random.default_rng(11)
    n, k, m = (dev(a) for a in make(g, [3], 4, metas=[(602, 627)]))
    v = dev(np.ones(1))
    table = torch.from_numpy(TABLE[:5].copy()).to(DEV)
    out, ent, bars, status = Guarded(1, 16), Guarded(1, 2, dtype=torch.float64), Guarded(1, 2, 16), Guarded(1)
    ok = dict(notes=n.data_ptr(), counts3=k.data_ptr(), meta=m.data_ptr(), valid=v.data_ptr(), table=table.data_ptr(), out=out.ptr, ent=ent.ptr,
              bars=bars.ptr, status=status.ptr, B=1, max_notes=4, max_bars=2)
    bad = [dict(notes=None), dict(counts3=None), dict(meta=None), dict(table=None), dict(out=None), dict(ent=None), dict(status=None),
           dict(B=0), dict(B=-1), dict(max_notes=0), dict(max_notes=32769), dict(max_bars=0), dict(max_bars=-1), dict(max_bars=513)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhm_structure_counts(*args.values(), _lib.current_stream()) == _lib.MH_ERR_INVALID, change
        assert b"structure_counts" in lib.mh_last_error()
    torch.cuda.synchronize()
    for buf in (out, ent, bars, status):
        assert (buf.get() == SENTINEL).all(), "a refused call writes nothing"
    for change in (dict(valid=None), dict(bars=None)):                  # what may be NULL
        args = {**ok, **change}
        assert lib.mhm_structure_counts(*args.values(), _lib.current_stream()) == 0, change
    torch.cuda.synchronize()
    assert status.get().tolist() == [sr.OK] and out.get()[0, :2].sum() == 3
    for kw in (dict(max_bars=513), dict(max_bars=0)):
        with pytest.raises(ValueError):
            metric.structure_counts_raw(n, k, m, **kw)
    with pytest.raises(ValueError):
        metric.structure_counts_raw(n, k[:, :2], m)


def test_512_generated_pieces_through_decode_tokens():
    tokens, masks, kinds = dr.make_batch(23, 320, (dr.BATCH_KINDS * 6)[:512])
    dec = du.decode_tokens(torch.from_numpy(tokens).to(DEV), torch.from_numpy(masks).to(DEV))
    sc = metric.structure_counts(dec, max_bars=12, return_bars=True)
    status = dec.status.cpu().numpy()
    want = sr.batch_counts(dec.notes.cpu().numpy(), dec.counts.cpu().numpy(), dec.meta.cpu().numpy(), metric.xlog2x_host(dec.notes.shape[1]),
                           status == dr.OK, 12)
    same(host(sc), want)
    ok = want["status"] == sr.OK
    c = want["counts"][ok]
    assert ok.sum() > 200 and (want["status"][status != dr.OK] == sr.MASKED).all()
    assert (c[:, 1] == 0).all() and np.array_equal(c[:, 0], dec.counts.cpu().numpy()[ok, 0]) and (c[:, 2] <= 12).all()
    assert c[:, 0].sum() > 3000 and c[:, 13].sum() > 200 and c[:, 9].sum() > 1000
    assert np.array_equal(want["bars"][ok][:, :, 0].sum(1), c[:, 0])
    h1 = want["entropy"][ok, 0].sum() / c[:, 12].sum()
    assert 0.5 < h1 < np.log2(12) and (c[:, 10] <= c[:, 11] * c[:, 9]).all()
