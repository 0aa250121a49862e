"""GPU: mha_interplay_counts (csrc/arrange.hip) through the C ABI, bit for bit against the plain-Python restatement
(tests/interplay_ref.py).  Every output buffer is sentinel-filled with a guard band on both sides and every element is compared.
Note counts around the 256-thread pass, the wave and the LDS tile T = mha_key_tile() (0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T,
T + 1, 2 T + 1, 600), three rows of 4096 notes; songs of 1, 2, 3, 16 and 17 rows; ids interleaved, negative, extreme, NULL; masks;
shifts up to 2^29 and one past it; every pitch distance 0..127; skipped notes; shuffled notes and shuffled rows; every status in one
batch; repeated bits; one launch; every refusal; 512 generated ComMU-shaped pieces through decode_tokens, four to a song."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import interplay_ref as ir  # noqa: E402
from gpu_helpers import SENTINEL, Guarded, library_launches  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402

DEV = "cuda"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]
NAMES = ("counts", "pairs", "ticks", "status")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def run(notes, counts3, meta, valid=None, song=None, shift=None):
    """mha_interplay_counts through the C ABI -> dict of numpy arrays, as interplay_ref.batch_counts"""
    B, max_notes = notes.shape[0], notes.shape[1]
    n, k, m = dev(notes), dev(counts3), dev(meta)
    v, s, h = (None if a is None else dev(a) for a in (valid, song, shift))
    out = dict(counts=Guarded(B, 8), pairs=Guarded(B, 9, dtype=torch.int64), ticks=Guarded(B, 9, dtype=torch.int64), status=Guarded(B))
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(_lib.lib().mha_interplay_counts(n.data_ptr(), k.data_ptr(), m.data_ptr(), p(v), p(s), p(h), out["counts"].ptr, out["pairs"].ptr,
                                               out["ticks"].ptr, out["status"].ptr, B, max_notes, _lib.current_stream()), "mha_interplay_counts")
    torch.cuda.synchronize()
    return {name: g.get() for name, g in out.items()}


def same(got, want, what=""):
    assert set(got) == set(NAMES)
    for name in NAMES:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def check(notes, counts3, meta, valid=None, song=None, shift=None, what=""):
    got = run(notes, counts3, meta, valid, song, shift)
    same(got, ir.batch_counts(notes, counts3, meta, valid, song, shift), what)
    return got


def junk(g, *shape):
    return g.integers(I32_MIN, I32_MAX, size=shape, endpoint=True).astype(np.int32)


def fill_row(g, notes, n, span=7680):
    """n notes into one row of a junk-filled list: starts inside `span` ticks, lengths up to 700 ticks (a few very long), pitches
    mostly in a five-octave band, hostile notes mixed in: pitches outside 0..127, starts before 0, ends at or before the start or
    behind 2^29"""
    start = g.integers(0, span, size=n)
    length = np.where(g.random(n) < 0.97, g.integers(1, 700, size=n), g.integers(60000, 200000, size=n))
    pitch = np.where(g.random(n) < 0.93, g.integers(30, 91, size=n), g.choice([-1, 128, I32_MIN, I32_MAX, 0, 127], size=n))
    end = start + length
    odd = g.random(n)
    start = np.where(odd < 0.02, -1 - g.integers(0, 50, size=n), start)
    end = np.where((odd >= 0.02) & (odd < 0.04), start - g.integers(0, 2, size=n), end)
    end = np.where((odd >= 0.04) & (odd < 0.05), 2 ** 29 + 1 + g.integers(0, 2, size=n), end)
    notes[:n, 0], notes[:n, 1], notes[:n, 2], notes[:n, 3] = start, end, pitch, g.integers(0, 128, size=n)


def make(g, ns, max_notes, span=7680):
    """one row per entry of ns -> notes, counts3, meta: everything outside a row's n notes is junk"""
    B = len(ns)
    notes, counts3 = junk(g, B, max_notes, 4), junk(g, B, 3)
    meta = junk(g, B, 11)
    meta[:, :3] = META[:3]
    for b in range(B):
        counts3[b, 0] = ns[b]
        fill_row(g, notes[b], ns[b], span)
    return notes, counts3, meta


# ------------------------------------------------------------------------------------------------------------------ the matrix
def test_note_counts_around_the_pass_the_wave_and_the_tile():
    T = _lib.lib().mha_key_tile()
    assert T == 512
    ns = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 600]
    g = np.random.default_rng(1)
    notes, counts3, meta = make(g, ns, 2 * T + 1)
    song = np.arange(len(ns)) % 2                                         # two songs of seven rows, interleaved
    got = check(notes, counts3, meta, song=song)
    assert (got["counts"][:, 0] + got["counts"][:, 1]).tolist() == ns and (got["status"] == ir.OK).all() and (got["counts"][:, 2] == 6).all()
    assert got["counts"][3:, 1].min() > 0 and got["pairs"][1:, :7].sum(1).min() > 0 and (got["pairs"][:, 7:] > 0).sum() >= 24, "the cases count something"
    assert not got["pairs"][0].any() and got["ticks"].max() > 2 ** 20 and (got["counts"][1:, 3] > 0).all()


def test_three_rows_of_4096_notes():
    g = np.random.default_rng(2)
    notes, counts3, meta = make(g, [4096] * 3, 4096, span=400000)
    got = check(notes, counts3, meta, shift=np.array([0, 1920, 77]))
    assert got["counts"][:, 0].min() > 3500 and got["pairs"][:, :7].sum() > 100000 and (got["status"] == ir.OK).all()


def test_songs_of_1_2_3_16_and_17_rows_under_every_kind_of_id():
    g = np.random.default_rng(3)
    sizes = [1, 2, 3, 16, 17]
    ids = [0, -1, I32_MIN, I32_MAX, 12345]
    song = np.concatenate([[i] * k for i, k in zip(ids, sizes)]).astype(np.int32)
    order = g.permutation(len(song))                                      # interleaved
    song = song[order]
    notes, counts3, meta = make(g, [int(x) for x in g.integers(5, 40, size=len(song))], 40)
    got = check(notes, counts3, meta, song=song)
    assert got["counts"][:, 2].tolist() == [sizes[ids.index(int(s))] - 1 for s in song]
    assert not got["pairs"][song == 0].any() and (got["pairs"][song != 0][:, :7].sum(1) > 0).all()
    one = check(notes, counts3, meta)                                     # song NULL: one song of 39 rows
    assert (one["counts"][:, 2] == 38).all() and one["pairs"].sum() > got["pairs"].sum()
    same(run(notes, counts3, meta, song=np.full(len(song), -3)), one, "one id for all")


def test_masks():
    g = np.random.default_rng(4)
    B = 12
    notes, counts3, meta = make(g, [30] * B, 32)
    song = np.arange(B) // 4
    for valid in (None, np.array([1] * 5 + [0] + [1] * 6), np.arange(B) % 2, np.where(song == 1, 0, 1), np.where(np.arange(B) % 3, -7, 0),
                  np.zeros(B, np.int32)):
        got = check(notes, counts3, meta, valid, song, what=None if valid is None else valid.tolist())
        on = np.ones(B, bool) if valid is None else np.asarray(valid) != 0
        assert got["status"].tolist() == np.where(on, ir.OK, ir.MASKED).tolist()
        assert got["counts"][:, 2].tolist() == [int(on[b]) * (int(on[song == song[b]].sum()) - 1) for b in range(B)]


def test_shifts():
    g = np.random.default_rng(5)
    notes, counts3, meta = make(g, [60] * 6, 64, span=3840)
    song = np.array([0, 0, 0, 1, 1, 1])
    plain = check(notes, counts3, meta, song=song, shift=np.zeros(6))
    same(run(notes, counts3, meta, song=song), plain, "shift NULL is no shift")
    bar = check(notes, counts3, meta, song=song, shift=np.array([0, 1920, 0, 2 ** 29, 2 ** 29, 2 ** 29]))
    assert not np.array_equal(bar["ticks"][:3], plain["ticks"][:3]) and np.array_equal(bar["ticks"][3:], plain["ticks"][3:]), "a common shift changes nothing"
    far = check(notes, counts3, meta, song=song, shift=np.array([0, 2 ** 29, 0, 0, 0, 2 ** 29 + 1]))
    assert far["status"].tolist() == [0, 0, 0, 0, 0, ir.BAD_SHIFT] and far["counts"][:, 2].tolist() == [2, 2, 2, 1, 1, 0] and not far["pairs"][1].any()
    neg = check(notes, counts3, meta, song=song, shift=np.array([-1, 0, 0, I32_MIN, I32_MAX, 0]))
    assert neg["status"].tolist() == [ir.BAD_SHIFT, 0, 0, ir.BAD_SHIFT, ir.BAD_SHIFT, 0]
    # the latest tick of all: end 2^29 shifted by 2^29
    notes[:, 0] = (2 ** 29 - 100, 2 ** 29, 60, 1)
    top = check(notes, counts3, meta, song=song, shift=np.array([2 ** 29, 2 ** 29 - 50, 2 ** 29 - 100, 0, 0, 0]))
    assert top["pairs"][0, 0] >= 1 and top["counts"][0, 3] >= 1


def test_every_pitch_distance():
    k = np.arange(128)
    rows = np.zeros((3, 128, 4), np.int32)
    rows[:, :, 0], rows[:, :, 1], rows[:, :, 3] = k * 100, k * 100 + 100, 64
    rows[0, :, 2], rows[1, :, 2], rows[2, :, 2] = 0, k, 127                # d = k between rows 0 and 1, 127 - k between 1 and 2
    counts3 = np.full((3, 3), 128, np.int32)
    got = check(rows, counts3, np.array([META] * 3, np.int32))
    ic = np.minimum(k % 12, 12 - k % 12)
    want = np.bincount(ic, minlength=7) + np.eye(7, dtype=np.int64)[5] * 128   # row 0 meets row 2 at d = 127 every time
    assert got["pairs"][0].tolist() == want.tolist() + [127 + 128, 0] and got["ticks"][0, 7] == 100 * 255
    assert got["pairs"][1, 7] == 127 and got["pairs"][1, 8] == 127 and got["pairs"][1, 0] == 2 * 11 and got["counts"][:, 3].tolist() == [128] * 3


def test_skipped_notes():
    good = (100, 200, 60, 1)
    bad = [(100, 200, -1, 1), (100, 200, 128, 1), (-1, 200, 60, 1), (I32_MIN, 200, 60, 1), (100, 100, 60, 1), (200, 100, 60, 1),
           (100, 2 ** 29 + 1, 60, 1), (100, I32_MAX, 60, 1), (I32_MAX, I32_MIN, 60, 1), (100, 200, I32_MIN, 1), (100, 200, I32_MAX, 1)]
    edge = [(0, 1, 0, 1), (0, 2 ** 29, 127, 1), (2 ** 29 - 1, 2 ** 29, 60, 1)]     # the last counted ones
    notes = np.array([bad + [good] + edge, [good] * 3 + bad + [good]], np.int64).astype(np.int32)
    got = check(notes, np.array([[15, I32_MIN, I32_MAX]] * 2, np.int32), np.array([META] * 2, np.int32))
    assert got["counts"].tolist() == [[4, 11, 1, 2, 0, 0, 0, 0], [4, 11, 1, 4, 0, 0, 0, 0]]
    assert got["pairs"][0].tolist() == [4, 0, 0, 0, 0, 4, 0, 0, 4] and got["ticks"][0, 0] == 400


def test_the_order_of_the_notes_and_of_the_rows_changes_no_bit():
    g = np.random.default_rng(8)
    ns = [600, 257, 31, 513, 90, 0, 300]
    notes, counts3, meta = make(g, ns, 600)
    song = np.array([3, 3, 9, 3, 9, 9, 9])
    shift = g.integers(0, 2000, size=7)
    first = check(notes, counts3, meta, song=song, shift=shift)
    for seed in (1, None):                                               # a shuffle, and the lists backwards
        shuffled = notes.copy()
        for b, n in enumerate(ns):
            shuffled[b, :n] = notes[b, :n][np.random.default_rng(seed).permutation(n) if seed else np.arange(n)[::-1]]
        assert not np.array_equal(shuffled, notes)
        same(run(shuffled, counts3, meta, song=song, shift=shift), first, "shuffled notes")
    for perm in (g.permutation(7), np.arange(7)[::-1]):
        got = run(notes[perm], counts3[perm], meta[perm], song=song[perm], shift=shift[perm])
        same(got, {k: v[perm] for k, v in first.items()}, "shuffled rows")


def test_every_status_inside_one_batch_over_junk_lists():
    g = np.random.default_rng(9)
    B = 16
    notes, counts3, meta = make(g, [20] * B, 24)
    song = np.array([0] * 8 + [1] * 4 + [2] * 4)
    valid = np.ones(B, np.int32)
    shift = np.zeros(B, np.int32)
    for b in (1, 2, 3, 4, 5, 6, 9, 14):                                   # refused rows hold junk, their counts are hostile
        notes[b] = junk(g, 24, 4)
    counts3[[1, 2, 3, 4], 0] = [-1, 25, I32_MIN, I32_MAX]
    shift[[5, 6]] = [-1, 2 ** 29 + 1]
    valid[9] = 0
    counts3[9, 0], shift[9] = -5, -5                                      # MASKED comes first
    counts3[14, 0], shift[14] = 99, -5                                    # BAD_COUNTS before BAD_SHIFT
    meta[13, 1] += 1                                                      # song 2: rows 12, 13 and 15 are mixed, 14 is out of range
    counts3[7, 0] = 24                                                    # a full list
    fill_row(g, notes[7], 24)
    got = check(notes, counts3, meta, valid, song, shift)
    C_, S_, M_, X_ = ir.BAD_COUNTS, ir.BAD_SHIFT, ir.MASKED, ir.MIXED
    assert got["status"].tolist() == [0, C_, C_, C_, C_, S_, S_, 0, 0, M_, 0, 0, X_, X_, C_, X_]
    refused = got["status"] != ir.OK
    assert not got["counts"][refused].any() and not got["pairs"][refused].any() and not got["ticks"][refused].any()
    assert got["counts"][[0, 7, 8, 10], 2].tolist() == [1, 1, 2, 2] and got["counts"][7, :2].sum() == 24
    meta[9, :3] += 1                                                      # a masked row's meta mixes nobody
    assert check(notes, counts3, meta, valid, song, shift)["status"].tolist() == got["status"].tolist()


@pytest.mark.parametrize("B", [1, 2, 65])
def test_batch_sizes_and_the_same_bits_on_a_repeated_call(B):
    g = np.random.default_rng(100 + B)
    notes, counts3, meta = make(g, [int(g.integers(0, 120)) for _ in range(B)], 120)
    song = g.integers(-2, 6, size=B)
    valid = (g.random(B) < 0.85).astype(np.int32)
    first = check(notes, counts3, meta, valid, song, g.integers(0, 3000, size=B) * 0 + 480)
    same(run(notes, counts3, meta, valid, song, np.full(B, 480)), first, "repeat")


def host(ic):
    return dict(counts=ic.counts.cpu().numpy(), pairs=ic.pairs.cpu().numpy(), ticks=ic.ticks.cpu().numpy(), status=ic.status.cpu().numpy())


def test_python_front_launches_once_whatever_the_batch():
    g = np.random.default_rng(11)
    seen = {}
    for B in (2, 64):
        arrays = make(g, [50] * B, 64)
        song, shift = np.arange(B) // 2, g.integers(0, 1000, size=B)
        notes, counts3, meta = (dev(a) for a in arrays)
        box = []
        seen[B] = library_launches(lambda: box.append(metric.interplay_counts_raw(notes, counts3, meta, None, dev(song), dev(shift))))
        ic = box[0]
        assert ic.counts.dtype == torch.int32 and ic.pairs.dtype == torch.int64 and ic.ticks.shape == (B, 9) and ic.counts.shape == (B, 8)
        same(host(ic), ir.batch_counts(*arrays, None, song, shift))
        plain = metric.interplay_counts_raw(notes, counts3, meta)
        same(host(plain), ir.batch_counts(*arrays))
        masked = metric.interplay_counts_raw(notes, counts3, meta, torch.arange(B, device=DEV) % 2 == 0, dev(song).long())
        same(host(masked), ir.batch_counts(*arrays, np.arange(B) % 2 == 0, song))
    assert seen[2] == seen[64] and len(seen[2]) == 1 and seen[2][0].startswith("interplay_counts_kernel"), seen


def test_every_refusal_leaves_the_outputs_alone():
    lib = _lib.lib()
    g = np.random.default_rng(12)
    n, k, m = (dev(a) for a in make(g, [3, 4], 4))
    v, s, h = dev(np.ones(2)), dev(np.zeros(2)), dev(np.zeros(2))
    counts, pairs, ticks, status = Guarded(2, 8), Guarded(2, 9, dtype=torch.int64), Guarded(2, 9, dtype=torch.int64), Guarded(2)
    ok = dict(notes=n.data_ptr(), counts3=k.data_ptr(), meta=m.data_ptr(), valid=v.data_ptr(), song=s.data_ptr(), shift=h.data_ptr(),
              counts=counts.ptr, pairs=pairs.ptr, ticks=ticks.ptr, status=status.ptr, B=2, max_notes=4)
    bad = [dict(notes=None), dict(counts3=None), dict(meta=None), dict(counts=None), dict(pairs=None), dict(ticks=None), dict(status=None),
           dict(B=0), dict(B=-1), dict(max_notes=0), dict(max_notes=-4), dict(max_notes=32769), dict(B=65537, max_notes=32768),
           dict(B=2 ** 31 - 1, max_notes=4)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mha_interplay_counts(*args.values(), _lib.current_stream()) == _lib.MH_ERR_INVALID, change
        assert b"interplay_counts" in lib.mh_last_error()
    torch.cuda.synchronize()
    for buf in (counts, pairs, ticks, status):
        assert (buf.get() == SENTINEL).all(), "a refused call writes nothing"
    for change in (dict(valid=None), dict(song=None), dict(shift=None), dict(valid=None, song=None, shift=None)):   # what may be NULL
        args = {**ok, **change}
        assert lib.mha_interplay_counts(*args.values(), _lib.current_stream()) == 0, change
    torch.cuda.synchronize()
    assert status.get().tolist() == [ir.OK] * 2 and counts.get()[:, :2].sum(1).tolist() == [3, 4] and counts.get()[:, 2].tolist() == [1, 1]
    with pytest.raises(ValueError):
        metric.interplay_counts_raw(n, k[:, :2], m)
    with pytest.raises(ValueError):
        metric.interplay_counts_raw(n, k, m, song=s[:1])


def test_512_generated_pieces_four_to_a_song():
    tokens, masks, kinds = dr.make_batch(23, 320, (dr.BATCH_KINDS * 6)[:512])
    dec = du.decode_tokens(torch.from_numpy(tokens).to(DEV), torch.from_numpy(masks).to(DEV))
    song = torch.arange(512, device=DEV, dtype=torch.int32) // 4
    # the generator draws every row's meta on its own: the even songs take their first row's tempo, key and time signature and inst 644
    even = (song % 2 == 0).unsqueeze(1)
    dec.meta[:, :3] = torch.where(even, dec.meta[(song * 4).long(), :3], dec.meta[:, :3])
    dec.meta[:, 5] = torch.where(torch.arange(512, device=DEV) % 16 == 2, 648, 644)          # and some rows are drums
    shift = torch.where(torch.arange(512, device=DEV) % 3 == 0, 1920, 0).to(torch.int32)
    status = dec.status.cpu().numpy()
    arrays = dec.notes.cpu().numpy(), dec.counts.cpu().numpy(), dec.meta.cpu().numpy()
    drums = arrays[2][:, 5] == 648
    for pitched_only in (True, False):
        ic = metric.interplay_counts(dec, song, shift=shift, pitched_only=pitched_only)
        valid = (status == dr.OK) & ~(drums & pitched_only)
        want = ir.batch_counts(*arrays, valid, song.cpu().numpy(), shift.cpu().numpy())
        same(host(ic), want)
        ok = want["status"] == ir.OK
        assert (want["status"][~valid] == ir.MASKED).all() and ok.sum() > 100 and (want["status"] == ir.MIXED).sum() > 50
        assert (want["counts"][ok, 1] == 0).all() and np.array_equal(want["counts"][ok, 0], arrays[1][ok, 0])
        assert want["pairs"][ok][:, :7].sum() > 3000 and want["counts"][ok, 3].sum() > 1000 and (want["counts"][ok, 2] >= 2).sum() > 30
    for s in range(0, 128, 2):
        rows = slice(4 * s, 4 * s + 4)
        p = want["pairs"][rows].sum(0)
        assert (p[:7] % 2 == 0).all() and p[7] == p[8]
