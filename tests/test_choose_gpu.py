"""GPU: mhac_pair_fit and mhac_choose (csrc/choose.hip) through the C ABI, bit for bit against the plain restatement
(tests/choose_ref.py).  Every output buffer is sentinel-filled with a guard band on both sides and every element is compared.
pair_fit: note counts around the 256-thread pass and the LDS tile T = mhac_key_tile() (0, 1, 255, 256, 257, T - 1, T, T + 1, 2 T + 1,
600), one song with rows of 4096 notes; the shapes (S, T, K) = (1,1,1), (1,2,1), (2,2,2), (1,3,3), (3,6,4), (1,2,16); masks; shifts up
to 2^29 and one past it; every pitch distance 0..127; skipped and shuffled notes; every status in one batch over junk lists; the
symmetry of a pair of rows; the K = 1 identity with mha_interplay_counts on the device; repeated bits; one launch.  choose, on
injected tables: (T, K) = (1,1), (2,2), (6,4), (16,2), (20,2) and (5,16) at the limit, (7,8) refused; more combinations than one
sweep of the block; negative tables; ties at the first and at the last q; a track without eligible rows in the first, a middle and
the last place, none eligible at all; +-2^40 and one beyond, read and unread; unary NULL and not; repeated bits; one launch.  Then
both kernels chained on 64 generated ComMU-shaped pieces through decode_tokens."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import choose_ref as cr  # noqa: E402
import decode_ref as dr  # noqa: E402
from gpu_helpers import SENTINEL, Guarded, library_launches  # noqa: E402
from musediffusion_amd import _lib, metric  # noqa: E402
from musediffusion_amd.utils import arrange_util as au, decode_util as du  # noqa: E402
from test_interplay_gpu import I32_MAX, I32_MIN, META, dev, fill_row, junk, make  # noqa: E402
from test_interplay_gpu import run as run_interplay  # noqa: E402

DEV = "cuda"
FIT_NAMES, CHOOSE_NAMES = ("ticks", "pairs", "status"), ("choice", "best", "first", "status")


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def p(t):
    return None if t is None else t.data_ptr()


def run_fit(notes, counts3, meta, S, T, K, valid=None, shift=None):
    """mhac_pair_fit through the C ABI -> dict of numpy arrays, as choose_ref.pair_fit"""
    B, R, max_notes = S * T * K, T * K, notes.shape[1]
    assert notes.shape[0] == B
    n, k, m = dev(notes), dev(counts3), dev(meta)
    v, h = (None if a is None else dev(a) for a in (valid, shift))
    out = dict(ticks=Guarded(B, R, 7, dtype=torch.int64), pairs=Guarded(B, R, 7, dtype=torch.int64), status=Guarded(B))
    _lib.check(_lib.lib().mhac_pair_fit(n.data_ptr(), k.data_ptr(), m.data_ptr(), p(v), p(h), out["ticks"].ptr, out["pairs"].ptr,
                                        out["status"].ptr, S, T, K, max_notes, _lib.current_stream()), "mhac_pair_fit")
    torch.cuda.synchronize()
    return {name: g.get() for name, g in out.items()}


def same(got, want, names, what=""):
    assert set(got) == set(names)
    for name in names:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def check_fit(notes, counts3, meta, S, T, K, valid=None, shift=None, what=""):
    got = run_fit(notes, counts3, meta, S, T, K, valid, shift)
    same(got, cr.pair_fit(notes, counts3, meta, S, T, K, valid, shift), FIT_NAMES, what)
    return got


def symmetric(got, S, T, K):
    """out[b, r] == out[partner, local(b)] for every pair of rows that are both OK; zeros on a row's own track"""
    R = T * K
    ok = got["status"] == cr.OK
    for name in ("ticks", "pairs"):
        a = got[name].reshape(S, R, R, 7)
        both = (ok.reshape(S, R, 1) & ok.reshape(S, 1, R))[..., None]
        assert np.array_equal(np.where(both, a, 0), np.where(both, a.transpose(0, 2, 1, 3), 0)), name
        for t in range(T):
            assert not a[:, t * K:(t + 1) * K, t * K:(t + 1) * K].any(), "the candidates of one track never meet"


# ------------------------------------------------------------------------------------------------------------------ pair_fit
def test_note_counts_around_the_pass_and_the_tile():
    T = _lib.lib().mhac_key_tile()
    assert T == 512
    ns = [0, 1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 600, 64, 300]
    g = np.random.default_rng(1)
    notes, counts3, meta = make(g, ns, 2 * T + 1)
    got = check_fit(notes, counts3, meta, 1, 6, 2)
    assert (got["status"] == cr.OK).all() and not got["pairs"][0].any() and not got["pairs"][:, 0].any()
    assert (got["pairs"][2:, 2:].reshape(10, 5, 2, 7).sum((2, 3)) > 0).sum() >= 10 * 4 and got["ticks"].max() > 2 ** 20, "the cases count something"
    symmetric(got, 1, 6, 2)


def test_one_song_with_rows_of_4096_notes():
    g = np.random.default_rng(2)
    notes, counts3, meta = make(g, [4096] * 2, 4096, span=400000)
    got = check_fit(notes, counts3, meta, 1, 2, 1, shift=np.array([0, 1920]))
    assert got["pairs"][0, 1].sum() > 30000 and (got["status"] == cr.OK).all()
    symmetric(got, 1, 2, 1)


@pytest.mark.parametrize("S, T, K", [(1, 1, 1), (1, 2, 1), (2, 2, 2), (1, 3, 3), (3, 6, 4), (1, 2, 16)])
def test_shapes_masks_and_the_same_bits_on_a_repeated_call(S, T, K):
    g = np.random.default_rng(100 + S * T * K)
    B = S * T * K
    notes, counts3, meta = make(g, [int(g.integers(0, 70)) for _ in range(B)], 70)
    valid = (g.random(B) < 0.85).astype(np.int32)
    shift = g.integers(0, 3, size=B) * 480
    first = check_fit(notes, counts3, meta, S, T, K, valid, shift)
    same(run_fit(notes, counts3, meta, S, T, K, valid, shift), first, FIT_NAMES, "repeat")
    symmetric(first, S, T, K)
    assert first["status"].tolist() == np.where(valid != 0, cr.OK, cr.MASKED).tolist()
    plain = check_fit(notes, counts3, meta, S, T, K)
    assert (plain["status"] == cr.OK).all() and (plain["pairs"].sum() > 0) == (T > 1)
    symmetric(plain, S, T, K)


def test_masks():
    g = np.random.default_rng(4)
    S, T, K = 2, 3, 2
    B = S * T * K
    notes, counts3, meta = make(g, [30] * B, 32)
    for valid in (np.array([1] * 5 + [0] + [1] * 6), np.arange(B) % 2, np.where(np.arange(B) < 6, 0, 1), np.where(np.arange(B) % 3, -7, 0),
                  np.zeros(B, np.int32)):
        got = check_fit(notes, counts3, meta, S, T, K, valid, what=valid.tolist())
        on = np.asarray(valid) != 0
        assert got["status"].tolist() == np.where(on, cr.OK, cr.MASKED).tolist()
        assert not got["pairs"][~on].any() and not got["pairs"].reshape(S, T * K, T * K, 7)[np.broadcast_to(~on.reshape(S, 1, T * K), (S, T * K, T * K))].any()


def test_shifts():
    g = np.random.default_rng(5)
    notes, counts3, meta = make(g, [60] * 6, 64, span=3840)
    plain = check_fit(notes, counts3, meta, 2, 3, 1, shift=np.zeros(6))
    same(run_fit(notes, counts3, meta, 2, 3, 1), plain, FIT_NAMES, "shift NULL is no shift")
    bar = check_fit(notes, counts3, meta, 2, 3, 1, shift=np.array([0, 1920, 0, 2 ** 29, 2 ** 29, 2 ** 29]))
    assert not np.array_equal(bar["ticks"][:3], plain["ticks"][:3]) and np.array_equal(bar["ticks"][3:], plain["ticks"][3:]), "a common shift changes nothing"
    far = check_fit(notes, counts3, meta, 2, 3, 1, shift=np.array([0, 2 ** 29, 0, 0, 0, 2 ** 29 + 1]))
    assert far["status"].tolist() == [0, 0, 0, 0, 0, cr.BAD_SHIFT] and not far["pairs"][1].any() and not far["pairs"][:, 2][3:].any()
    neg = check_fit(notes, counts3, meta, 2, 3, 1, shift=np.array([-1, 0, 0, I32_MIN, I32_MAX, 0]))
    assert neg["status"].tolist() == [cr.BAD_SHIFT, 0, 0, cr.BAD_SHIFT, cr.BAD_SHIFT, 0]
    notes[:, 0] = (2 ** 29 - 100, 2 ** 29, 60, 1)                          # the latest tick of all: end 2^29 shifted by 2^29
    top = check_fit(notes, counts3, meta, 2, 3, 1, shift=np.array([2 ** 29, 2 ** 29 - 50, 2 ** 29 - 100, 0, 0, 0]))
    assert top["pairs"][0, 1, 0] >= 1


def test_every_pitch_distance():
    k = np.arange(128)
    rows = np.zeros((3, 128, 4), np.int32)
    rows[:, :, 0], rows[:, :, 1], rows[:, :, 3] = k * 100, k * 100 + 100, 64
    rows[0, :, 2], rows[1, :, 2], rows[2, :, 2] = 0, k, 127                # d = k between rows 0 and 1, 127 - k between 1 and 2
    got = check_fit(rows, np.full((3, 3), 128, np.int32), np.array([META] * 3, np.int32), 1, 3, 1)
    ic = np.minimum(k % 12, 12 - k % 12)
    assert got["pairs"][0, 1].tolist() == np.bincount(ic, minlength=7).tolist() == got["pairs"][1, 0].tolist()
    assert got["pairs"][0, 2].tolist() == [0, 0, 0, 0, 0, 128, 0] and got["ticks"][0, 2, 5] == 12800 and not got["pairs"][0, 0].any()


def test_skipped_and_shuffled_notes():
    good = (100, 200, 60, 1)
    bad = [(100, 200, -1, 1), (100, 200, 128, 1), (-1, 200, 60, 1), (I32_MIN, 200, 60, 1), (100, 100, 60, 1), (200, 100, 60, 1),
           (100, 2 ** 29 + 1, 60, 1), (100, I32_MAX, 60, 1), (I32_MAX, I32_MIN, 60, 1), (100, 200, I32_MIN, 1), (100, 200, I32_MAX, 1)]
    edge = [(0, 1, 0, 1), (0, 2 ** 29, 127, 1), (2 ** 29 - 1, 2 ** 29, 60, 1)]     # the last counted ones
    notes = np.array([bad + [good] + edge, [good] * 3 + bad + [good]], np.int64).astype(np.int32)
    got = check_fit(notes, np.array([[15, I32_MIN, I32_MAX]] * 2, np.int32), np.array([META] * 2, np.int32), 1, 2, 1)
    assert got["pairs"][0, 1].tolist() == [4, 0, 0, 0, 0, 4, 0] and got["ticks"][0, 1, 0] == 400
    g = np.random.default_rng(8)
    ns = [600, 257, 31, 513, 90, 0, 300, 40]
    notes, counts3, meta = make(g, ns, 600)
    shift = g.integers(0, 2000, size=8)
    first = check_fit(notes, counts3, meta, 1, 4, 2, shift=shift)
    for seed in (1, None):                                               # a shuffle, and the lists backwards
        shuffled = notes.copy()
        for b, n in enumerate(ns):
            shuffled[b, :n] = notes[b, :n][np.random.default_rng(seed).permutation(n) if seed else np.arange(n)[::-1]]
        assert not np.array_equal(shuffled, notes)
        same(run_fit(shuffled, counts3, meta, 1, 4, 2, shift=shift), first, FIT_NAMES, "shuffled notes")


def test_every_status_inside_one_batch_over_junk_lists():
    g = np.random.default_rng(9)
    S, T, K = 2, 4, 2
    B = S * T * K
    notes, counts3, meta = make(g, [20] * B, 24)
    valid, shift = np.ones(B, np.int32), np.zeros(B, np.int32)
    for b in (1, 2, 3, 4, 5, 6):                                           # refused rows hold junk, their counts are hostile
        notes[b] = junk(g, 24, 4)
    counts3[[1, 2, 3], 0] = [-1, 25, I32_MIN]
    shift[[4, 5]] = [-1, 2 ** 29 + 1]
    valid[6] = 0
    counts3[6, 0], shift[6] = -5, -5                                       # MASKED comes first
    counts3[7, 0] = 24                                                     # a full list
    fill_row(g, notes[7], 24)
    meta[9, 1] += 1                                                        # song 1: row 9 (track 0) is odd - every row of another track is mixed, and so is it
    counts3[15, 0], shift[15] = 99, -5                                     # BAD_COUNTS before BAD_SHIFT
    got = check_fit(notes, counts3, meta, S, T, K, valid, shift)
    C_, S_, M_, X_ = cr.BAD_COUNTS, cr.BAD_SHIFT, cr.MASKED, cr.MIXED
    assert got["status"].tolist() == [0, C_, C_, C_, S_, S_, M_, 0, 0, X_, X_, X_, X_, X_, X_, C_]
    refused = got["status"] != cr.OK
    assert not got["ticks"][refused].any() and not got["pairs"][refused].any()
    assert got["pairs"][0, 7].sum() > 0 and got["pairs"][8].sum() > 0 and not got["pairs"][8, 1].any(), "row 8 meets the rows of the other tracks, MIXED or not"
    meta[6, :3] += 1                                                       # a masked row's meta mixes nobody
    assert check_fit(notes, counts3, meta, S, T, K, valid, shift)["status"].tolist() == got["status"].tolist()


def test_at_one_candidate_the_sums_are_the_interplay_counts_of_the_device():
    g = np.random.default_rng(10)
    S, T = 5, 4
    B = S * T
    notes, counts3, meta = make(g, [int(g.integers(0, 300)) for _ in range(B)], 300)
    valid = (g.random(B) < 0.9).astype(np.int32)
    shift = g.integers(0, 4, size=B) * 480
    meta[13, 0] += 1                                                       # one song is mixed
    valid[12:16] = 1
    fit = run_fit(notes, counts3, meta, S, T, 1, valid, shift)
    whole = run_interplay(notes, counts3, meta, valid, np.arange(B) // T, shift)
    assert np.array_equal(fit["status"], whole["status"]) and (fit["status"] == cr.MIXED).sum() >= 3
    assert np.array_equal(fit["ticks"].sum(1), whole["ticks"][:, :7]) and np.array_equal(fit["pairs"].sum(1), whole["pairs"][:, :7])
    assert whole["pairs"][:, :7].sum() > 10000


def test_python_front_launches_once_whatever_the_batch():
    g = np.random.default_rng(11)
    seen = {}
    for S in (1, 8):
        T, K = 3, 2
        B = S * T * K
        arrays = make(g, [50] * B, 64)
        shift = g.integers(0, 1000, size=B)
        notes, counts3, meta = (dev(a) for a in arrays)
        box = []
        seen[S] = library_launches(lambda: box.append(metric.pair_fit_raw(notes, counts3, meta, S, T, K, None, dev(shift))))
        fit = box[0]
        assert fit.ticks.dtype == torch.int64 and fit.ticks.shape == (B, T * K, 7) == fit.pairs.shape and fit.status.dtype == torch.int32
        got = dict(ticks=fit.ticks.cpu().numpy(), pairs=fit.pairs.cpu().numpy(), status=fit.status.cpu().numpy())
        same(got, cr.pair_fit(*arrays, S, T, K, None, shift), FIT_NAMES)
        W = metric.fit_scores(fit.ticks, (3, -1, -1, 2, 2, 1, -4))
        assert W.is_cuda and np.array_equal(W.cpu().numpy(), cr.fit_scores(got["ticks"], (3, -1, -1, 2, 2, 1, -4)))
    assert seen[1] == seen[8] and len(seen[1]) == 1 and seen[1][0].startswith("pair_fit_kernel"), seen


def test_a_refused_pair_fit_leaves_the_outputs_alone():
    lib = _lib.lib()
    g = np.random.default_rng(12)
    n, k, m = (dev(a) for a in make(g, [3, 4], 4))
    ticks, pairs, status = Guarded(2, 2, 7, dtype=torch.int64), Guarded(2, 2, 7, dtype=torch.int64), Guarded(2)
    ok = dict(notes=n.data_ptr(), counts3=k.data_ptr(), meta=m.data_ptr(), valid=None, shift=None, ticks=ticks.ptr, pairs=pairs.ptr,
              status=status.ptr, S=1, T=2, K=1, max_notes=4)
    for change in (dict(notes=None), dict(status=None), dict(S=0), dict(T=21), dict(K=17), dict(max_notes=0), dict(max_notes=32769),
                   dict(S=2 ** 29 + 1)):
        assert lib.mhac_pair_fit(*{**ok, **change}.values(), _lib.current_stream()) == _lib.MH_ERR_INVALID, change
    torch.cuda.synchronize()
    for buf in (ticks, pairs, status):
        assert (buf.get() == SENTINEL).all(), "a refused call writes nothing"
    assert lib.mhac_pair_fit(*ok.values(), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert status.get().tolist() == [0, 0] and not ticks.get()[0, 0].any() and not ticks.get()[1, 1].any()


# ------------------------------------------------------------------------------------------------------------------ choose
def run_choose(W, S, T, K, unary=None, eligible=None):
    """mhac_choose through the C ABI -> dict of numpy arrays, as choose_ref.choose"""
    w = dev64(W)
    u = None if unary is None else dev64(unary)
    e = None if eligible is None else dev(eligible)
    out = dict(choice=Guarded(S, T), best=Guarded(S, dtype=torch.int64), first=Guarded(S, dtype=torch.int64), status=Guarded(S))
    _lib.check(_lib.lib().mhac_choose(w.data_ptr(), p(u), p(e), out["choice"].ptr, out["best"].ptr, out["first"].ptr, out["status"].ptr,
                                      S, T, K, _lib.current_stream()), "mhac_choose")
    torch.cuda.synchronize()
    return {name: g.get() for name, g in out.items()}


def check_choose(W, S, T, K, unary=None, eligible=None, what=""):
    got = run_choose(W, S, T, K, unary, eligible)
    same(got, cr.choose(W, S, T, K, unary, eligible), CHOOSE_NAMES, what)
    assert (got["best"] >= got["first"]).all()
    return got


@pytest.mark.parametrize("T, K, S", [(1, 1, 3), (2, 2, 3), (6, 4, 3), (16, 2, 2), (20, 2, 1), (5, 16, 2)])
def test_tables_up_to_the_limit(T, K, S):
    g = np.random.default_rng(T * 100 + K)
    R = T * K
    W = g.integers(-10 ** 6, 10 ** 6, size=(S, R, R))                     # negative entries too
    unary = g.integers(-10 ** 5, 10 ** 5, size=(S, R))
    eligible = np.ones((S, R), np.int32)
    others = [r for r in range(R) if r % K]                               # candidate 0 stays: every track is kept
    if others:
        eligible[-1, g.choice(others, size=(len(others) + 2) // 3, replace=False)] = 0
    first = check_choose(W, S, T, K, unary, eligible)
    same(run_choose(W, S, T, K, unary, eligible), first, CHOOSE_NAMES, "repeat")
    assert (first["status"] == cr.CH_OK).all() and (first["choice"] >= 0).all()
    if K ** T > 256:
        assert (first["choice"] > 0).any() and (first["best"] > first["first"]).all(), "more combinations than one sweep of the block"
    if K ** T >= 1 << 18:                                                 # the restatement of 2^20 combinations takes seconds: once
        return
    plain = check_choose(W, S, T, K)                                      # unary and eligible NULL
    assert (plain["status"] == cr.CH_OK).all()
    all_negative = check_choose(-np.abs(W) - 1, S, T, K)
    assert (all_negative["best"] < 0).all() or T == 1


def test_seven_tracks_of_eight_candidates_are_refused():
    lib = _lib.lib()
    w = dev64(np.zeros((1, 56, 56)))
    out = dict(choice=Guarded(1, 7), best=Guarded(1, dtype=torch.int64), first=Guarded(1, dtype=torch.int64), status=Guarded(1))
    args = (w.data_ptr(), None, None, out["choice"].ptr, out["best"].ptr, out["first"].ptr, out["status"].ptr, 1, 7, 8, _lib.current_stream())
    assert lib.mhac_choose(*args) == _lib.MH_ERR_UNSUPPORTED and b"1048576" in lib.mh_last_error()
    torch.cuda.synchronize()
    for buf in out.values():
        assert (buf.get() == SENTINEL).all(), "a refused call writes nothing"
    with pytest.raises(_lib.MuseHipError, match="1048576"):
        metric.choose_tracks(w, 1, 7, 8)


def test_ties_at_the_first_and_at_the_last_combination():
    T, K = 6, 4                                                           # 4096 combinations: sixteen sweeps of the block
    R = T * K
    W = np.zeros((4, R, R), np.int64)
    got = check_choose(W, 4, T, K)                                        # every combination ties: q = 0
    assert not got["choice"].any() and not got["best"].any()
    last = [t * K + K - 1 for t in range(T)]
    for t in range(T):
        for u in range(t + 1, T):
            W[1, last[t], last[u]] = 3                                    # the last q alone is best
            W[2, last[t], last[u]] = 3
            W[2, t * K, u * K] = 3                                        # the first and the last q tie: the first
            W[3, last[u], last[t]] = 9                                    # the higher track first: never read
    W[3, 5, 9] = W[3, 6, 9] = 1                                           # q = 1 + 4 and q = 2 + 4 tie (with any digits above: the smallest are zeros)
    got = check_choose(W, 4, T, K)
    assert got["choice"].tolist() == [[0] * T, [K - 1] * T, [0] * T, [0, 1, 1, 0, 0, 0]] and got["best"].tolist() == [0, 45, 45, 1]
    assert got["first"].tolist() == [0, 0, 45, 0]
    un = np.zeros((4, R), np.int64)
    un[:, last] = 1                                                       # now the last q wins song 2 as well
    assert check_choose(W, 4, T, K, un)["choice"][2].tolist() == [K - 1] * T


def test_tracks_without_eligible_rows_and_none_at_all():
    g = np.random.default_rng(21)
    T, K = 5, 3
    R = T * K
    W = g.integers(-50, 50, size=(6, R, R))
    unary = g.integers(-5, 5, size=(6, R))
    eligible = (g.random((6, R)) < 0.8).astype(np.int32)
    eligible[:, ::K] = 1
    eligible[0, :K] = 0                                                   # the first track
    eligible[1, 2 * K:3 * K] = 0                                          # a middle one
    eligible[2, -K:] = 0                                                  # the last
    eligible[3, :K] = eligible[3, -K:] = 0
    eligible[4] = 0                                                       # none at all
    eligible[5] = 0
    eligible[5, 2 * K + 1] = 1                                            # one row of one track
    got = check_choose(W, 6, T, K, unary, eligible)
    assert got["status"].tolist() == [cr.CH_PARTIAL] * 4 + [cr.CH_EMPTY, cr.CH_PARTIAL]
    assert (got["choice"] == -1).tolist() == [[True, False, False, False, False], [False, False, True, False, False], [False, False, False, False, True],
                                              [True, False, False, False, True], [True] * 5, [True, True, False, True, True]]
    assert got["choice"][5, 2] == 1 and got["best"][5] == unary[5, 2 * K + 1] == got["first"][5] and (got["best"][4], got["first"][4]) == (0, 0)
    check_choose(W, 6, T, K, None, eligible)


def test_scores_at_and_beyond_the_limit_read_and_unread():
    T, K = 3, 2
    R = T * K
    big = 2 ** 40
    W = np.zeros((8, R, R), np.int64)
    unary = np.zeros((8, R), np.int64)
    eligible = np.ones((8, R), np.int32)
    W[0, 0, 2], W[0, 1, 5] = big, -big                                    # at the limit: fine
    W[1, 0, 2] = big + 1                                                  # beyond, and read
    W[2, 2, 0] = big + 1                                                  # beyond, the higher track first: unread
    W[3, 0, 1] = -big - 1                                                 # beyond, within one track: unread
    W[4, 0, 2] = -big - 1                                                 # beyond, but row 0 is ineligible: unread
    eligible[4, 0] = 0
    unary[5, 3] = -big - 1                                                # unary beyond, and read
    unary[6, 3] = big + 1                                                 # unary beyond, row 3 ineligible: unread
    eligible[6, 3] = 0
    W[7, 2, 5] = np.iinfo(np.int64).min                                   # as far beyond as it gets, track 1 left out: unread
    eligible[7, 2:4] = 0
    got = check_choose(W, 8, T, K, unary, eligible)
    B_ = cr.CH_BAD_SCORE
    assert got["status"].tolist() == [0, B_, 0, 0, 0, B_, 0, cr.CH_PARTIAL]
    assert got["choice"][[1, 5]].tolist() == [[-1] * 3] * 2 and not got["best"][[1, 5]].any() and not got["first"][[1, 5]].any()
    assert got["best"][0] == big and got["choice"][0].tolist() == [0, 0, 0]
    full = np.full((1, R, R), big, np.int64)                              # every term at the limit: three terms, exact
    assert check_choose(full, 1, T, K, np.full((1, R), big))["best"].tolist() == [6 * big]
    assert check_choose(-full, 1, T, K, np.full((1, R), -big))["best"].tolist() == [-6 * big]
    assert check_choose(W[:7], 7, T, K)["status"].tolist() == [0, B_, 0, 0, B_, 0, 0], "unary and eligible NULL"


def test_choose_front_launches_once_whatever_the_batch():
    g = np.random.default_rng(23)
    seen = {}
    T, K = 4, 3
    for S in (1, 65):
        W = g.integers(-100, 100, size=(S, T * K, T * K))
        unary = g.integers(-10, 10, size=(S, T * K))
        eligible = g.random((S, T * K)) < 0.7
        box = []
        seen[S] = library_launches(lambda: box.append(metric.choose_tracks(dev64(W), S, T, K, dev64(unary), torch.from_numpy(eligible).to(DEV))))
        res = box[0]
        assert res.choice.dtype == torch.int32 and res.choice.shape == (S, T) and res.best.dtype == torch.int64 and res.status.shape == (S,)
        got = dict(choice=res.choice.cpu().numpy(), best=res.best.cpu().numpy(), first=res.first.cpu().numpy(), status=res.status.cpu().numpy())
        same(got, cr.choose(W, S, T, K, unary, eligible), CHOOSE_NAMES)
    assert seen[1] == seen[65] and len(seen[1]) == 1 and seen[1][0].startswith("choose_kernel"), seen


# ------------------------------------------------------------------------------------------------------------------ chained
def test_both_kernels_chained_on_64_generated_pieces():
    S, T, K = 4, 4, 4
    tokens, masks, kinds = dr.make_batch(31, 320, (dr.BATCH_KINDS * 6)[:64])
    dec = du.decode_tokens(torch.from_numpy(tokens).to(DEV), torch.from_numpy(masks).to(DEV))
    row = torch.arange(64, device=DEV)
    # the generator draws every row's meta on its own: three songs take their first row's tempo, key and time signature
    same_song = (row // 16 < 3).unsqueeze(1)
    dec.meta[:, :3] = torch.where(same_song, dec.meta[(row // 16 * 16), :3], dec.meta[:, :3])
    dec.meta[:, 5] = torch.where(row % 16 == 9, 648, 644)                 # and one row a song is a drum row
    shift = au.anchor_shift(dec)
    ok = dec.status == du.OK
    valid = ok & (dec.meta[:, 5] != metric.DRUMS_INST)
    fit = metric.pair_fit(dec, S, T, K, shift=shift, valid=valid)
    W = metric.fit_scores(fit.ticks)
    res = metric.choose_tracks(W, S, T, K, eligible=ok.view(S, T * K))
    arrays = dec.notes.cpu().numpy(), dec.counts.cpu().numpy(), dec.meta.cpu().numpy()
    want = cr.pair_fit(*arrays, S, T, K, valid.cpu().numpy(), shift.cpu().numpy())
    same(dict(ticks=fit.ticks.cpu().numpy(), pairs=fit.pairs.cpu().numpy(), status=fit.status.cpu().numpy()), want, FIT_NAMES)
    assert (want["status"][:48] == cr.OK).sum() > 20 and want["pairs"].sum() > 1000 and (want["status"] == cr.MASKED).sum() >= 4
    want_W = cr.fit_scores(want["ticks"])
    assert np.array_equal(W.cpu().numpy(), want_W) and (want_W < 0).any() and (want_W > 0).any()
    chosen = cr.choose(want_W, S, T, K, None, ok.cpu().numpy().reshape(S, T * K))
    same(dict(choice=res.choice.cpu().numpy(), best=res.best.cpu().numpy(), first=res.first.cpu().numpy(), status=res.status.cpu().numpy()),
         chosen, CHOOSE_NAMES)
    assert (chosen["best"] > chosen["first"]).any() and (chosen["status"] <= cr.CH_PARTIAL).all()
