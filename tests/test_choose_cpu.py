"""CPU: choosing each song's tracks among candidates without a device.  tests/choose_ref.py (the plain restatement of
csrc/choose.hip and of metric.fit_scores) on hand-made songs with answers worked out here; its enumeration against an
itertools.product brute force on random small tables with planted ties and ineligible rows; every status; best >= first; at K = 1
the pair ticks summed over the partners are tests/interplay_ref.py's class columns; metric.fit_scores on host tensors;
utils.arrange_util.anchor_shift on host tensors and candidate_batch's refusals; the extension header musehip_choose.h against the
compiler and against both libraries' exports, as tests/test_abi_cpu.py does for the headers of _lib.HEADERS; the refusals of the
entry points, which come before any launch.  No kernel runs here: the device side is tests/test_choose_gpu.py and
tests/test_choose_sampling_gpu.py."""
import ctypes as C
import itertools
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import choose_ref as cr
import interplay_ref as ir
from musediffusion_amd import _abi, _lib, metric
from musediffusion_amd.utils import arrange_util as au, decode_util as du
from test_abi_cpu import cls, compile_check, header_unit

META = [580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727]   # 100 bpm, c major, 4/4
HEADER = "musehip_choose.h"


def batch_of(rows, metas=None):
    """rows: lists of (start, end, pitch, velocity), in the candidate layout -> notes, counts3, meta arrays"""
    cap = max(1, max(len(r) for r in rows))
    notes = np.zeros((len(rows), cap, 4), np.int32)
    for b, r in enumerate(rows):
        notes[b, :len(r)] = np.array(r, np.int64).reshape(-1, 4)
    counts3 = np.array([[len(r), 0, 0] for r in rows], np.int32)
    return notes, counts3, np.array(metas if metas is not None else [META] * len(rows), np.int32)


# ------------------------------------------------------------------------------------------------------------------ hand-made songs
def test_a_fifth_against_a_tritone_candidate():
    """track 0: one c4; track 1: candidate 0 an f sharp (a tritone, class 6), candidate 1 a g (a fifth, class 5) - T = 2, K = 2, so
    track 0 has two candidates as well: the same c4 twice"""
    c4, fs, g = [(0, 480, 60, 90)], [(240, 960, 66, 90)], [(240, 960, 67, 90)]
    out = cr.pair_fit(*batch_of([c4, c4, fs, g]), 1, 2, 2)
    assert out["status"].tolist() == [0] * 4
    e = lambda c: [240 if i == c else 0 for i in range(7)]  # noqa: E731
    z = [0] * 7
    assert out["ticks"].tolist() == [[z, z, e(6), e(5)], [z, z, e(6), e(5)], [e(6), e(6), z, z], [e(5), e(5), z, z]]
    assert (out["pairs"] == out["ticks"] // 240).all()
    W = cr.fit_scores(out["ticks"])
    assert W.tolist() == [[[0, 0, -480, 240], [0, 0, -480, 240], [-480, -480, 0, 0], [240, 240, 0, 0]]]
    got = cr.choose(W, 1, 2, 2)
    assert got["choice"].tolist() == [[0, 1]] and got["best"].tolist() == [240] and got["first"].tolist() == [-480] and got["status"].tolist() == [cr.CH_OK]
    # the fifth ineligible: what is left is the tritone; weights of the caller turn the choice round
    assert cr.choose(W, 1, 2, 2, eligible=[[1, 1, 1, 0]])["choice"].tolist() == [[0, 0]]
    assert cr.choose(cr.fit_scores(out["ticks"], (0, 0, 0, 0, 0, -1, 3)), 1, 2, 2)["choice"].tolist() == [[0, 0]]


def test_touching_notes_the_clamp_and_the_same_track():
    a, b = [(0, 480, 60, 1), (960, 1000, 60, 1)], [(480, 960, 64, 1)]
    out = cr.pair_fit(*batch_of([a, b]), 1, 2, 1)
    assert not out["ticks"].any() and not out["pairs"].any() and out["status"].tolist() == [0, 0], "notes that only touch"
    out = cr.pair_fit(*batch_of([[(0, 481, 60, 1), (959, 1000, 60, 1)], b]), 1, 2, 1)
    assert out["ticks"][0, 1].tolist() == [0, 0, 0, 0, 2, 0, 0] == out["ticks"][1, 0].tolist() and out["pairs"][0, 1, 4] == 2
    out = cr.pair_fit(*batch_of([[(0, 65536, 60, 1), (0, 2 ** 29, 60, 1)], [(0, 2 ** 29, 61, 1)]]), 1, 2, 1)
    assert out["ticks"][0, 1, 1] == 2 * 65535 == out["ticks"][1, 0, 1] and out["pairs"][1, 0, 1] == 2, "a pair adds 65535 ticks at most"
    # the same two rows as the two candidates of ONE track: they never meet; as two songs: neither
    same = [(0, 100, 60, 1)], [(0, 100, 64, 1)]
    for shape in ((1, 1, 2), (2, 1, 1)):
        out = cr.pair_fit(*batch_of(same), *shape)
        assert not out["ticks"].any() and not out["pairs"].any() and out["status"].tolist() == [0, 0], shape
    out = cr.pair_fit(*batch_of(same), 1, 2, 1)
    assert out["ticks"][:, :, 4].tolist() == [[0, 100], [100, 0]]
    # T = 2, K = 2: a row meets both candidates of the other track and neither of its own; a shift moves a row
    out = cr.pair_fit(*batch_of([same[0], same[0], same[1], same[1]]), 1, 2, 2, shift=[0, 50, 0, 100])
    assert out["ticks"][:, :, 4].tolist() == [[0, 0, 100, 0], [0, 0, 50, 50], [100, 50, 0, 0], [0, 50, 0, 0]]


def test_every_status_of_the_pair_fit():
    a, b = [(0, 100, 60, 1)], [(0, 100, 64, 1)]
    out = cr.pair_fit(*batch_of([a, b, a]), 1, 3, 1, valid=[1, 0, 1])
    assert out["status"].tolist() == [0, cr.MASKED, 0] and not out["ticks"][1].any() and not out["ticks"][:, 1].any()
    assert out["ticks"][0, 2, 0] == 100, "a masked row is nobody's partner"
    assert cr.pair_fit(*batch_of([a, b]), 1, 2, 1, shift=[0, -1])["status"].tolist() == [0, cr.BAD_SHIFT]
    assert cr.pair_fit(*batch_of([a, b]), 1, 2, 1, shift=[2 ** 29 + 1, 2 ** 29])["status"].tolist() == [cr.BAD_SHIFT, 0]
    notes, counts3, meta = batch_of([a, b, a])
    counts3[:, 0] = [1, 2, -1]
    assert cr.pair_fit(notes, counts3, meta, 1, 3, 1)["status"].tolist() == [0, cr.BAD_COUNTS, cr.BAD_COUNTS]
    odd = [META, META[:1] + [603] + META[2:], META, META]
    # MIXED compares with partners only: the odd row is a candidate of track 0, so the rows of track 1 are mixed and so is it, while
    # its fellow candidate is not - the two never meet
    out = cr.pair_fit(*batch_of([a, a, b, b], odd), 1, 2, 2)
    assert out["status"].tolist() == [0, cr.MIXED, cr.MIXED, cr.MIXED] and not out["ticks"][1:].any()
    assert out["ticks"][0, :, 4].tolist() == [0, 0, 100, 100], "whether a partner is itself MIXED plays no part"
    out = cr.pair_fit(*batch_of([a, a, b, b], odd), 1, 2, 2, valid=[1, 0, 1, 1])
    assert out["status"].tolist() == [0, cr.MASKED, 0, 0] and out["ticks"][0, 2, 4] == 100
    out = cr.pair_fit(*batch_of([a, a, b, b], odd), 2, 1, 2)
    assert out["status"].tolist() == [0] * 4, "candidates of one track are no partners"
    # the order: MASKED before BAD_COUNTS before BAD_SHIFT before MIXED
    notes, counts3, meta = batch_of([a, b], odd[:2][::-1])
    counts3[0, 0] = 9
    assert cr.pair_fit(notes, counts3, meta, 1, 2, 1, valid=[0, 1], shift=[-1, 0])["status"].tolist() == [cr.MASKED, 0]
    assert cr.pair_fit(notes, counts3, meta, 1, 2, 1, shift=[-1, 0])["status"].tolist() == [cr.BAD_COUNTS, 0]
    counts3[0, 0] = 1
    assert cr.pair_fit(notes, counts3, meta, 1, 2, 1, shift=[-1, 0])["status"].tolist() == [cr.BAD_SHIFT, 0]
    assert cr.pair_fit(notes, counts3, meta, 1, 2, 1)["status"].tolist() == [cr.MIXED, cr.MIXED]


def random_batch(g, B, cap):
    notes = np.zeros((B, cap, 4), np.int32)
    notes[:, :, 0] = g.integers(0, 3000, size=(B, cap))
    notes[:, :, 1] = notes[:, :, 0] + g.integers(1, 700, size=(B, cap))
    notes[:, :, 2] = g.integers(40, 80, size=(B, cap))
    counts3 = np.zeros((B, 3), np.int32)
    counts3[:, 0] = g.integers(cap // 2, cap + 1, size=B)
    return notes, counts3, np.array([META] * B, np.int32)


def test_at_one_candidate_the_pair_ticks_sum_to_the_interplay_columns():
    g = np.random.default_rng(5)
    S, T = 3, 4
    notes, counts3, meta = random_batch(g, S * T, 30)
    shift = g.integers(0, 500, size=S * T)
    valid = np.ones(S * T, np.int32)
    valid[5] = 0
    out = cr.pair_fit(notes, counts3, meta, S, T, 1, valid, shift)
    want = ir.batch_counts(notes, counts3, meta, valid, np.arange(S * T) // T, shift)
    assert np.array_equal(out["status"], want["status"]) and want["pairs"].sum() > 500
    assert np.array_equal(out["ticks"].sum(1), want["ticks"][:, :7]) and np.array_equal(out["pairs"].sum(1), want["pairs"][:, :7])
    for s in range(S):                                                    # a pair of rows is seen alike from both sides
        block = out["ticks"][s * T:(s + 1) * T]
        assert np.array_equal(block, block.transpose(1, 0, 2))


# ------------------------------------------------------------------------------------------------------------------ the search
def brute(W, T, K, unary, eligible):
    """one song, by itertools.product over the candidates of the kept tracks: (choice, best, first, status)"""
    R = T * K
    el = [[eligible is None or eligible[t * K + k] != 0 for k in range(K)] for t in range(T)]
    kept = [t for t in range(T) if any(el[t])]
    if not kept:
        return [-1] * T, 0, 0, cr.CH_EMPTY
    found = []
    for ks in itertools.product(*[[k for k in range(K) if el[t][k]] for t in kept]):
        rows = [t * K + k for t, k in zip(kept, ks)]
        terms = [0 if unary is None else int(unary[r]) for r in rows] + [int(W[rows[i]][rows[j]]) for i in range(len(rows)) for j in range(i + 1, len(rows))]
        if any(abs(v) > cr.SCORE_MAX for v in terms):
            return [-1] * T, 0, 0, cr.CH_BAD_SCORE
        found.append((sum(k * K ** t for t, k in zip(kept, ks)), sum(terms), ks))
    found.sort()
    top = max(v for _, v, _ in found)
    ks = next(ks for _, v, ks in found if v == top)
    choice = [-1] * T
    for t, k in zip(kept, ks):
        choice[t] = k
    return choice, top, found[0][1], cr.CH_OK if len(kept) == T else cr.CH_PARTIAL


def random_table(g, T, K):
    """W, unary, eligible of one song: small values, so that ties are common; now and then a whole track ineligible, everything
    ineligible, or an entry beyond 2^40 somewhere"""
    R = T * K
    W = g.integers(-3, 4, size=(R, R)).astype(np.int64)
    unary = None if g.random() < 0.3 else g.integers(-2, 3, size=R).astype(np.int64)
    eligible = None if g.random() < 0.3 else (g.random(R) < 0.7).astype(np.int32)
    if eligible is not None and g.random() < 0.3:
        eligible[int(g.integers(T)) * K:][:K] = 0
    if eligible is not None and g.random() < 0.05:
        eligible[:] = 0
    if g.random() < 0.3:
        W[:] = int(g.integers(-2, 3))                                     # every combination ties
    if g.random() < 0.3:                                                  # anywhere, the half of the table that is never read included
        W[int(g.integers(R)), int(g.integers(R))] = int(g.choice([2 ** 40, -2 ** 40, 2 ** 40 + 1, -2 ** 40 - 1, 2 ** 62]))
    return W, unary, eligible


def test_the_enumeration_against_brute_force_on_300_tables():
    g = np.random.default_rng(11)
    seen, moved = set(), 0
    for _ in range(300):
        T, K = int(g.integers(1, 5)), int(g.integers(1, 4))
        W, unary, eligible = random_table(g, T, K)
        got = cr.choose(W[None], 1, T, K, None if unary is None else unary[None], None if eligible is None else eligible[None])
        choice, best, first, status = brute(W, T, K, unary, eligible)
        assert (got["choice"][0].tolist(), int(got["best"][0]), int(got["first"][0]), int(got["status"][0])) == (choice, best, first, status)
        assert got["best"][0] >= got["first"][0]
        seen.add(status)
        moved += best > first
    assert seen == {cr.CH_OK, cr.CH_PARTIAL, cr.CH_EMPTY, cr.CH_BAD_SCORE} and moved > 50


def test_every_status_of_the_search_and_its_ties():
    T, K = 3, 2
    W = np.zeros((1, 6, 6), np.int64)
    W[0, 1, 3] = W[0, 0, 4] = 5                                           # q = 1 + 2 = 3 (k = 1, 1, 0) and q = 0 + 0 + 0 with r = 0, 4?  no: r 4 is k = 0
    got = cr.choose(W, 1, T, K)
    assert got["choice"].tolist() == [[0, 0, 0]] and got["best"].tolist() == [5] and got["first"].tolist() == [5], "the tie goes to the smallest q"
    W[0, 0, 4] = 4
    assert cr.choose(W, 1, T, K)["choice"].tolist() == [[1, 1, 0]]
    W[0, 3, 1] = 100                                                      # the higher track first: never read
    assert cr.choose(W, 1, T, K)["best"].tolist() == [5]
    got = cr.choose(W, 1, T, K, eligible=[[1, 1, 0, 0, 1, 1]])
    assert got["status"].tolist() == [cr.CH_PARTIAL] and got["choice"].tolist() == [[0, -1, 0]] and got["best"].tolist() == [4]
    got = cr.choose(W, 1, T, K, eligible=[[0] * 6])
    assert (got["status"].tolist(), got["choice"].tolist(), got["best"].tolist(), got["first"].tolist()) == ([cr.CH_EMPTY], [[-1] * 3], [0], [0])
    W[0, 0, 2] = 2 ** 40
    assert cr.choose(W, 1, T, K)["status"].tolist() == [cr.CH_OK] and cr.choose(W, 1, T, K)["best"].tolist() == [2 ** 40 + 4]
    W[0, 0, 2] = -2 ** 40 - 1
    got = cr.choose(W, 1, T, K)
    assert (got["status"].tolist(), got["choice"].tolist(), got["best"].tolist(), got["first"].tolist()) == ([cr.CH_BAD_SCORE], [[-1] * 3], [0], [0])
    assert cr.choose(W, 1, T, K, eligible=[[0, 1, 1, 1, 1, 1]])["status"].tolist() == [cr.CH_OK], "an entry that no admissible q reads"
    assert cr.choose(W, 1, T, K, eligible=[[1, 1, 0, 0, 1, 1]])["status"].tolist() == [cr.CH_PARTIAL]
    W[0, 0, 2] = 0
    un = np.array([[0, 0, 0, 0, 0, 2 ** 40 + 1]], np.int64)
    assert cr.choose(W, 1, T, K, un)["status"].tolist() == [cr.CH_BAD_SCORE]
    assert cr.choose(W, 1, T, K, un, [[1, 1, 1, 1, 1, 0]])["status"].tolist() == [cr.CH_OK]
    un[0, 5] = 7
    got = cr.choose(W, 1, T, K, un)
    assert got["choice"].tolist() == [[1, 1, 1]] and got["best"].tolist() == [12] and got["first"].tolist() == [4]


def test_names_and_limits_mirror_the_header():
    enums = _lib.EXTENSION_ABI[HEADER].enums
    assert enums == {"MHAC_OK": 0, "MHAC_PARTIAL": 1, "MHAC_EMPTY": 2, "MHAC_BAD_SCORE": 3, "MHAC_MAX_TRACKS": 20, "MHAC_MAX_CANDIDATES": 16,
                     "MHAC_MAX_COMBINATIONS": 2 ** 20}
    assert (metric.CHOOSE_OK, metric.CHOOSE_PARTIAL, metric.CHOOSE_EMPTY, metric.CHOOSE_BAD_SCORE) == (cr.CH_OK, cr.CH_PARTIAL, cr.CH_EMPTY, cr.CH_BAD_SCORE)
    assert (cr.OK, cr.MASKED, cr.BAD_COUNTS, cr.BAD_SHIFT, cr.MIXED) == (metric.INTERPLAY_OK, metric.INTERPLAY_MASKED, metric.INTERPLAY_BAD_COUNTS,
                                                                         metric.INTERPLAY_BAD_SHIFT, metric.INTERPLAY_MIXED)
    assert metric.DEFAULT_FIT_WEIGHTS == cr.DEFAULT_WEIGHTS == (0, -2, -2, 1, 1, 1, -2)
    assert (metric.FIT_SCORE_MAX, metric.FIT_WEIGHT_MAX, metric.CHOOSE_MAX_COMBINATIONS) == (cr.SCORE_MAX, cr.WEIGHT_MAX, cr.MAX_COMBINATIONS)


def test_fit_scores_on_host_tensors():
    g = np.random.default_rng(13)
    ticks = g.integers(0, 10 ** 6, size=(12, 6, 7)).astype(np.int64)
    ticks[0, 1] = 2 ** 46                                                 # what a pair of rows holds at most: the clamp at +-2^40
    ticks[1, 0, 1] = 2 ** 46
    for weights in (None, (0, -2, -2, 1, 1, 1, -2), (1024, -1024, 0, 7, -7, 1, 1), [0] * 7):
        got = metric.fit_scores(torch.from_numpy(ticks), weights)
        assert got.dtype == torch.int64 and got.shape == (2, 6, 6)
        assert np.array_equal(got.numpy(), cr.fit_scores(ticks, cr.DEFAULT_WEIGHTS if weights is None else weights)), weights
    assert metric.fit_scores(torch.from_numpy(ticks))[0, 1, 0].item() == -2 ** 40 and metric.fit_scores(torch.from_numpy(ticks), [1] * 7)[0, 0, 1].item() == 2 ** 40
    w = torch.tensor([3, 0, 0, 0, 0, 0, -1])
    assert torch.equal(metric.fit_scores(torch.from_numpy(ticks), w), metric.fit_scores(torch.from_numpy(ticks), (3, 0, 0, 0, 0, 0, -1)))
    for bad in (dict(weights=(1,) * 6), dict(weights=(1025,) + (0,) * 6), dict(weights=(0,) * 6 + (-1025,)), dict(weights=torch.zeros(6)),
                dict(ticks=torch.zeros(4, 2, 6, dtype=torch.int64)), dict(ticks=torch.zeros(5, 2, 7, dtype=torch.int64)),
                dict(ticks=torch.zeros(4, 2, 7, dtype=torch.int32))):
        args = dict(ticks=torch.zeros(4, 2, 7, dtype=torch.int64), weights=None)
        args.update(bad)
        with pytest.raises(ValueError):
            metric.fit_scores(**args)


# ------------------------------------------------------------------------------------------------------------------ the utilities
def test_anchor_shift_on_host_tensors_and_the_refusals_of_candidate_batch():
    bar_first, note_first = [2, 140, 300, 60, 400], [140, 300, 60, 400, 2]
    ts = lambda t: META[:2] + [t] + META[3:]  # noqa: E731
    rows = [bar_first, note_first, bar_first, bar_first, bar_first, [], bar_first, bar_first]
    metas = [ts(627), ts(627), ts(628), ts(629), ts(630), ts(627), ts(626), ts(627)]
    status = [0, 0, 0, 0, 0, 0, 0, du.NO_EOS]
    L = max(len(r) for r in rows)
    restored = torch.zeros(len(rows), L, dtype=torch.int32)
    for b, r in enumerate(rows):
        restored[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
    dec = SimpleNamespace(restored=restored, lengths=torch.tensor([len(r) for r in rows], dtype=torch.int32),
                          meta=torch.tensor(metas, dtype=torch.int32), status=torch.tensor(status, dtype=torch.int32))
    got = au.anchor_shift(dec)
    assert got.dtype == torch.int32 and got.tolist() == [1920, 0, 1440, 1440, 2880, 1920, 0, 0]
    # on the decoded rows of one song it differs from align_shift by one constant: 0 with a late row, one bar without
    for song_rows in ([0, 1], [0, 5]):
        sub = SimpleNamespace(restored=restored[song_rows], lengths=dec.lengths[song_rows], meta=dec.meta[song_rows], status=dec.status[song_rows])
        diff = (au.anchor_shift(sub) - au.align_shift(sub, torch.zeros(2, dtype=torch.int32))).tolist()
        assert diff == ([0, 0] if song_rows == [0, 1] else [1920, 1920])
    base = dict(bpm=100)
    for bad in (dict(tracks=[]), dict(n_songs=0), dict(candidates=0), dict(tracks=[dict(bpm=90)])):
        args = dict(tracks=[dict()], n_songs=1, candidates=2)
        args.update(bad)
        with pytest.raises(ValueError):
            au.candidate_batch(base, args["tracks"], args["n_songs"], 64, args["candidates"], "cpu")


# ------------------------------------------------------------------------------------------------------------------ the extension header
P, I = C.c_void_p, C.c_int
PINS = {"mhac_pair_fit": (I, [P] * 8 + [I] * 4 + [P]), "mhac_key_tile": (I, []), "mhac_choose": (I, [P] * 7 + [I] * 3 + [P])}


def exports(path, pattern):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and re.match(pattern, ln.split()[-1])}


def test_the_extension_tables_stand_beside_the_pinned_ones():
    assert _lib.EXTENSION_HEADERS == (HEADER,) and list(_lib.EXTENSION_ABI) == [HEADER] and HEADER not in _lib.HEADERS and HEADER not in _lib.ABI
    d = _lib.EXTENSION_ABI[HEADER]
    ref = _abi.load(HEADER, _abi.load("musehip.h"))
    assert list(d.protos) == list(ref.protos) == list(PINS) and d.enums == ref.enums and not d.structs
    assert all(d.protos[n] == PINS[n] for n in PINS)
    assert list(_lib.EXTENSION_SIGNATURES) == list(PINS) and all(_lib.EXTENSION_SIGNATURES[n] is d.protos[n] for n in PINS)
    # no name shared with another table, and the prefix is the family's alone: two letters, which the one-letter pattern does not claim
    assert not set(_lib.EXTENSION_SIGNATURES) & (set(_lib.PRODUCT_SIGNATURES) | set(_lib.DBG_SIGNATURES))
    assert all(n.startswith("mhac_") and not re.match(r"mh[a-z]?_", n) for n in PINS)
    assert all(k.startswith("MHAC_") for k in d.enums)
    with pytest.raises(_abi.AbiError, match="mhac_key_tile"):
        _lib._merged((_lib.EXTENSION_SIGNATURES, {"mhac_key_tile": 1}))


def test_the_header_against_both_libraries_exports():
    code = re.sub(r"/\*.*?\*/", " ", open(_abi.INCLUDE_DIR + "/" + HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mhac_[a-z0-9_]+)\s*\(", code))
    assert declared == set(PINS)
    assert exports(_lib.LIB_PATH, r"mhac_") == declared == exports(_lib.DBG_LIB_PATH, r"mhac_")
    assert not exports(_lib.LIB_PATH, r"mh[a-z]{2,}_") - declared, "no other prefix of two letters"
    handle = _lib.lib()
    for name, (res, args) in _lib.EXTENSION_SIGNATURES.items():
        fn = getattr(handle, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert handle.mhac_key_tile() == 512 == handle.mha_key_tile()
    with _lib.debug_library() as dbg:
        assert dbg is not handle and all(hasattr(dbg, n) for n in PINS) and dbg.mhac_key_tile() == 512
        assert list(dbg.mhac_choose.argtypes) == PINS["mhac_choose"][1]
    assert _lib.lib() is handle


def test_compiler_agrees_with_the_extension_header_and_catches_a_wrong_table(tmp_path):
    d = _lib.EXTENSION_ABI[HEADER]
    lines = ['static_assert(MHA_MIXED == 4, "the header brings enum mha_status with it");']
    r = compile_check(header_unit(HEADER, d.structs, d.protos, d.enums, lines), tmp_path / "abi.cpp")
    assert r.returncode == 0, r.stderr[-4000:]
    wrong = {n: (res, list(args)) for n, (res, args) in d.protos.items()}
    assert cls(C.c_int64) != cls(wrong["mhac_pair_fit"][1][8])
    wrong["mhac_pair_fit"][1][8] = C.c_int64                              # S is an int
    r = compile_check(header_unit(HEADER, {}, wrong), tmp_path / "abi_wrong.cpp")
    assert r.returncode != 0 and "mhac_pair_fit: argument 8" in r.stderr and "mhac_pair_fit: argument 7" not in r.stderr and "mhac_choose" not in r.stderr
    wrong = {n: (res, list(args)) for n, (res, args) in d.protos.items()}
    wrong["mhac_choose"][1].append(C.c_int)
    r = compile_check(header_unit(HEADER, {}, wrong), tmp_path / "abi_arity.cpp")
    assert r.returncode != 0 and "mhac_choose: arity" in r.stderr and "mhac_pair_fit" not in r.stderr
    r = compile_check(header_unit(HEADER, {}, {}, {"MHAC_BAD_SCORE": 2}), tmp_path / "abi_enum_wrong.cpp")
    assert r.returncode != 0 and "MHAC_BAD_SCORE" in r.stderr


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_argument_checks_need_no_device():
    """the refusals come before any launch: MH_ERR_INVALID or MH_ERR_UNSUPPORTED and a text"""
    lib = _lib.lib()
    buf = (C.c_int64 * 64)()
    a = C.addressof(buf)
    ok = dict(notes=a, counts3=a, meta=a, valid=a, shift=a, ticks=a, pairs=a, status=a, S=1, T=2, K=2, max_notes=4)
    bad = [dict(notes=None), dict(counts3=None), dict(meta=None), dict(ticks=None), dict(pairs=None), dict(status=None), dict(S=0), dict(S=-1),
           dict(T=0), dict(T=21), dict(K=0), dict(K=17), dict(T=-1), dict(max_notes=0), dict(max_notes=-1), dict(max_notes=32769),
           dict(S=16385, max_notes=32768), dict(S=2 ** 29, max_notes=1), dict(S=2 ** 31 - 1, T=20, K=16, max_notes=1), dict(S=2 ** 27 + 1, max_notes=4)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhac_pair_fit(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"pair_fit" in lib.mh_last_error()
    ok = dict(W=a, unary=a, eligible=a, choice=a, best=a, first=a, status=a, S=1, T=2, K=2)
    bad = [dict(W=None), dict(choice=None), dict(best=None), dict(first=None), dict(status=None), dict(S=0), dict(S=-3), dict(T=0), dict(T=21),
           dict(K=0), dict(K=17), dict(K=-1)]
    for change in bad:
        args = {**ok, **change}
        assert lib.mhac_choose(*args.values(), None) == _lib.MH_ERR_INVALID, change
        assert b"choose" in lib.mh_last_error()
    for T, K in ((7, 8), (20, 3), (6, 16), (11, 4), (20, 16)):
        assert lib.mhac_choose(*{**ok, "T": T, "K": K}.values(), None) == _lib.MH_ERR_UNSUPPORTED, (T, K)
        assert b"1048576" in lib.mh_last_error() and b"exact" in lib.mh_last_error()
    assert not any(buf), "a refused call writes nothing"
    # the Python fronts refuse the same before they touch the library or ask for a device
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    z64 = lambda *s: torch.zeros(*s, dtype=torch.int64)  # noqa: E731
    for call in (lambda: metric.pair_fit_raw(z(4, 4, 3), z(4, 3), z(4, 11), 1, 2, 2),
                 lambda: metric.pair_fit_raw(z(3, 4, 4), z(3, 3), z(3, 11), 1, 2, 2),
                 lambda: metric.pair_fit_raw(z(4, 4, 4), z(4, 2), z(4, 11), 1, 2, 2),
                 lambda: metric.pair_fit_raw(z(4, 4, 4), z(4, 3), z(3, 11), 1, 2, 2),
                 lambda: metric.pair_fit_raw(z(4, 4, 4), z(4, 3), z(4, 11), 1, 2, 2, shift=z(3)),
                 lambda: metric.pair_fit_raw(z(4, 4, 4), z(4, 3), z(4, 11), 0, 2, 2),
                 lambda: metric.pair_fit_raw(z(21, 4, 4), z(21, 3), z(21, 11), 1, 21, 1),
                 lambda: metric.pair_fit_raw(z(17, 4, 4), z(17, 3), z(17, 11), 1, 1, 17),
                 lambda: metric.pair_fit_raw(z(1, 32769, 4), z(1, 3), z(1, 11), 1, 1, 1),
                 lambda: metric.choose_tracks(z64(1, 4, 3), 1, 2, 2),
                 lambda: metric.choose_tracks(z(1, 4, 4), 1, 2, 2),
                 lambda: metric.choose_tracks(z64(1, 4, 4), 1, 2, 2, unary=z64(1, 3)),
                 lambda: metric.choose_tracks(z64(1, 4, 4), 1, 2, 2, eligible=z(2, 4)),
                 lambda: metric.choose_tracks(z64(1, 4, 4), 1, 0, 2)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.MuseHipError):
        metric.pair_fit_raw(z(4, 4, 4), z(4, 3), z(4, 11), 1, 2, 2)         # host tensors: there is no CPU path
    with pytest.raises(_lib.MuseHipError):
        metric.choose_tracks(z64(1, 4, 4), 1, 2, 2)
