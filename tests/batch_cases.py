"""The edge cases of the batch, validator and metric kernels (csrc/batch.hip), shared by tools/make_golden_batch_edges.py (which runs
the reference on the short ones), tests/test_batch_cases_cpu.py (oracle against that fixture, and the conditions on this list) and
tests/test_batch_matrix_gpu.py (every kernel through the C ABI).  Not a conftest: plain numpy, no GPU, no fixtures.

A family is one entry point; a family is a list of batches; a batch is a dict of launch parameters plus `rows`; a row is a dict with a
`name`, its inputs and - where the answer is not simply the oracle's - what the kernel is documented to do with it.  Rows of at most
STORE_MAX tokens are `stored`: the reference itself ran on them and tests/golden/batch_edges.npz holds what it returned or raised.
Longer rows are regenerated from their name (the seed) and checked against oracle/batch.py.

Token classes: 0 pad, 1 EOS, 2 BAR, 3..130 pitch, 131..194 velocity, 195..303 chord, 304..431 duration, 432..559 position, 560.. meta.
"""
import zlib

import numpy as np

from oracle import batch as ob

I32, F32 = np.int32, np.float32
MAX_ROW = 4096           # mh_batch_max_row(): the LDS-resident kernels' row limit
TB = 256                 # their chunk: a row is scanned 256 tokens at a time with a carried rank
STORE_MAX = 300          # rows up to this length go through the reference into the fixture
M2B_WRAP = (9, 116537)   # B x L = 4096 blocks x 256 threads + 257 elements: the grid-stride loop's second sweep, and a ragged end
assert M2B_WRAP[0] * M2B_WRAP[1] == 4096 * 256 + 257

ENTRY = {"mt": "mh_corrupt_masking_token", "mn": "mh_corrupt_masking_note", "rn": "mh_corrupt_randomize_note",
         "rr": "mh_corrupt_random_rotating", "r2p": "mh_ragged_to_padded", "m2b": "mh_meta_to_batch", "val": "mh_validate_tokens",
         "msim": "mh_msim_vectors", "ctrl": "mh_controllability_counts"}

# exception classes of the reference as the fixture stores them
EXC = {"none": 0, "AssertionError": 1, "IndexError": 2, "ValueError": 3, "UnboundLocalError": 4, "SequenceToMidiError": 5,
       "RuntimeError": 6, "KeyError": 7, "other": 8}


def exc_code(e):
    return EXC.get(type(e).__name__, EXC["other"])


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _meta(rng):
    return list(rng.integers(560, 729, 11)) + [0]


def ragged(rows, key="seq", dtype=I32, width=None):
    """rows -> (values back to back, offsets int64 [B + 1]); per-token inputs (u: [n], new: [n, 3]) share the offsets"""
    lens = [len(r["seq"]) for r in rows]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    parts = [np.asarray(r[key], dtype) for r in rows]
    shape = (0,) if width is None else (0, width)
    vals = np.concatenate(parts) if parts else np.zeros(shape, dtype)
    return vals.astype(dtype), off


# ------------------------------------------------------------------------------------------------------------- masking_token
def _mt_row(name, n, eos=(), u=None):
    rng = _rng("mt/" + name)
    seq = rng.integers(2, 560, n).astype(I32)
    m = np.array(_meta(rng), I32)
    seq[:min(n, 12)] = m[:min(n, 12)]
    for e in eos:
        seq[e] = 1
    u = rng.random(n).astype(F32) if u is None else np.asarray(u(n, rng), F32)
    return {"name": name, "seq": seq, "u": u, "stored": n <= STORE_MAX}


def mt_batches():
    p32 = F32(0.3)
    below = np.nextafter(p32, F32(0))

    def on_p(n, rng):     # draws exactly on float32(p) (strict compare: kept) next to the float just below it (masked)
        u = np.full(n, p32, F32)
        u[1::2] = below
        return u
    rows = [
        _mt_row("len0", 0), _mt_row("len5", 5), _mt_row("len12", 12), _mt_row("len13_eos12", 13, [12]), _mt_row("len13_noeos", 13),
        _mt_row("eos12", 40, [12]), _mt_row("eos_last_268", 268, [267]), _mt_row("eos267", 300, [267]), _mt_row("eos268", 300, [268]),
        _mt_row("eos269", 300, [269]), _mt_row("eos_before12_only", 40, [5]), _mt_row("eos_before12_and_after", 40, [3, 25]),
        _mt_row("no_eos", 40), _mt_row("no_eos_268", 268), _mt_row("two_eos", 40, [20, 30]), _mt_row("eos_at_11_and_12", 40, [11, 12]),
        _mt_row("draw_on_p", 60, [59], on_p), _mt_row("len4096_eos_last", 4096, [4095]), _mt_row("len4096_noeos", 4096),
        _mt_row("len4096_eos_4094", 4096, [4094]), _mt_row("len1", 1),
    ]
    zero = lambda n, rng: np.where(rng.random(n) < 0.5, 0.0, rng.random(n))
    top = lambda n, rng: np.where(rng.random(n) < 0.5, np.nextafter(F32(1), F32(0)), rng.random(n))
    return [
        {"name": "p0.3", "p": 0.3, "rows": rows},
        {"name": "p0", "p": 0.0, "rows": [_mt_row("p0_a", 50, [49], zero), _mt_row("p0_empty", 0), _mt_row("p0_b", 270, [269], zero)]},
        {"name": "p1", "p": 1.0, "rows": [_mt_row("p1_a", 50, [49], top), _mt_row("p1_b", 270, [268], top), _mt_row("p1_noeos", 30, (), top)]},
        {"name": "B1", "p": 0.3, "rows": [_mt_row("single", 70, [69])]},
        {"name": "B1_empty", "p": 0.3, "rows": [_mt_row("single_empty", 0)]},
    ]


# --------------------------------------------------------------------------------------------------- masking_note / randomize_note
NEVER = 2.0              # a draw that fires for no p


def _note_row(name, n, vel, fire=None, dense=None):
    """n tokens without velocity tokens, then velocity tokens at `vel`.  fire: None = random draws; else the positions whose token
    fires - every other draw slot holds NEVER, so a kernel that indexed the draws by position instead of rank would not fire them."""
    rng = _rng("note/" + name)
    pool = np.concatenate([np.arange(2, 131), np.arange(195, 560)])
    seq = rng.choice(pool, n).astype(I32) if n else np.zeros(0, I32)
    if dense is not None:
        vel = np.nonzero(rng.random(n) < dense)[0]
    vel = [v for v in vel if 0 <= v < n]
    seq[vel] = rng.integers(131, 195, len(vel))
    elig = ob._eligible_velocity(seq)
    if fire is None:
        u = rng.random(n).astype(F32)
    else:
        u = np.full(n, NEVER, F32)
        for k, idx in enumerate(elig):
            if fire == "all" or idx in fire:
                u[k] = 0.25
        if fire == "all":
            u[:] = 0.25      # slots past the eligible count too: a token at n-2 / n-1 that consumed one would fire
    new = np.stack([rng.integers(131, 195, n), rng.integers(3, 131, n), rng.integers(304, 432, n)], 1).astype(I32).reshape(n, 3)
    return {"name": name, "seq": seq, "u": u, "new": new, "vel": vel, "stored": n <= STORE_MAX}


def note_batches():
    """shared by masking_note and randomize_note (p = 0.5)"""
    n6 = 600
    edge = [
        _note_row("vel0", 20, [0], [0]), _note_row("vel1", 20, [1], [1]), _note_row("vel0_and_1", 20, [0, 1], [0, 1]),
        _note_row("n3_vel0_fires", 3, [0], [0]), _note_row("n3_vel0_quiet", 3, [0], []), _note_row("n4_vel0_fires", 4, [0], [0]),
        _note_row("n3_all_vel", 3, [0, 1, 2], "all"), _note_row("n2_vel", 2, [0, 1], "all"), _note_row("n1_vel", 1, [0], "all"),
        _note_row("seam_all", n6, [254, 255, 256, 257], [254, 255, 256, 257]), _note_row("seam_255", n6, [100, 255], [255]),
        _note_row("seam_256", n6, [100, 256], [256]), _note_row("seam_254_257", n6, [254, 255, 256, 257], [254, 257]),
        _note_row("seam_253", n6, [7, 253], [253]), _note_row("seam_257", n6, [7, 257, 258], [257]),
        _note_row("seam_512", n6, [30, 300, 511, 512, 513], [511, 513]), _note_row("seam_512_mid", n6, [511, 512, 513], [512]),
        _note_row("tail_eligible", 40, [10, 37], [37]), _note_row("tail_not_eligible", 40, [38, 39], "all"),
        _note_row("tail_mixed", 258, [255, 256, 257], "all"), _note_row("overlap_pairs", 64, [10, 11, 12, 20, 22, 30, 33], "all"),
        _note_row("ordinary_a", 90, [], None, dense=0.25), _note_row("empty_between", 0, []), _note_row("ordinary_b", 130, [], None, dense=0.25),
        _note_row("all_vel_256", 256, range(256)), _note_row("all_vel_257", 257, range(257)), _note_row("all_vel_4096", 4096, range(4096)),
        _note_row("dense_1000", 1000, [], None, dense=0.3), _note_row("dense_4096", 4096, [], None, dense=0.25),
        _note_row("sparse_4096", 4096, [0, 255, 256, 2047, 2048, 4093, 4094, 4095], "all"),
        _note_row("no_vel", 300, []),
    ]
    return [{"name": "edges", "p": 0.5, "rows": edge},
            {"name": "B1", "p": 0.5, "rows": [_note_row("single", 77, [], None, dense=0.25)]},
            {"name": "p1", "p": 1.0, "rows": [_note_row("p1_a", 270, [], None, dense=0.5), _note_row("p1_all_vel", 260, range(260))]}]


# ------------------------------------------------------------------------------------------------------------- random_rotating
# status the kernel documents (csrc/batch.hip, data/corruption.py): 0 rotated as the reference rotates; 1 flagged; 2 longer than MAX_ROW
RR_FLAGGED = ("one_bar", "no_bar", "no_eos", "eos_before_second_bar", "pair_second_out_of_range", "pair_first_negative",
              "pair_unsorted", "pair_equal", "len4097", "c0_one_bar")


def rr_status(seq, pairs):
    """the documented status of one row, from the rules and not from the kernel"""
    if len(seq) > MAX_ROW:
        return 2
    bars = np.nonzero(seq == 2)[0]
    eos = np.nonzero(seq == 1)[0]
    if len(bars) < 2 or len(eos) == 0:
        return 1
    for first, second in pairs:
        if first < 0 or second <= first or second >= len(bars):
            return 1
        b2e = bars[second + 1] if second < len(bars) - 1 else eos[-1]
        if b2e < bars[second]:
            return 1
    return 0


def _bar_row(name, bar_lens, pairs, eos=True, tail=0, prefix=12, eos_at=None):
    rng = _rng("rr/" + name)
    seq = _meta(rng)[:prefix]
    for bl in bar_lens:
        seq += [2] + list(rng.integers(3, 560, bl))
    if eos:
        seq.append(1)
    seq += list(rng.integers(3, 560, tail))
    seq = np.array(seq, I32)
    if eos_at is not None:
        seq[eos_at] = 1
    pairs = np.array(pairs, I32).reshape(-1, 2)
    nbar = int((seq == 2).sum())
    legal = all(0 <= f < s and (s < nbar or nbar < 2) for f, s in pairs)      # what random.sample(range(nbar), 2), sorted, can return
    return {"name": name, "seq": seq, "pairs": pairs, "status": rr_status(seq, pairs), "stored": len(seq) <= STORE_MAX and legal}


def _many_bars(name, pairs):
    """4096 tokens: 12 meta, 2100 bars (1983 of one token, 117 empty, shuffled by the seed), EOS"""
    rng = _rng("rr/" + name)
    lens = np.array([1] * 1983 + [0] * 117)
    rng.shuffle(lens)
    r = _bar_row(name, list(lens), pairs)
    assert len(r["seq"]) == MAX_ROW and int((r["seq"] == 2).sum()) == 2100
    return r


def rr_batches():
    c3 = [
        _bar_row("ordinary", [8, 12, 4, 16, 8], [(0, 3), (1, 2), (2, 4)]),
        _bar_row("adjacent", [8, 12, 4, 16], [(0, 1), (1, 2), (2, 3)]),
        _bar_row("one_bar", [20], [(0, 1)] * 3),
        _bar_row("last_bar_second", [8, 12, 4, 16], [(0, 3), (2, 3), (1, 3)]),
        _bar_row("same_pair", [8, 12, 4, 16], [(1, 3)] * 3),
        _bar_row("no_eos", [8, 8, 8], [(0, 1)] * 3, eos=False),
        _bar_row("two_bars", [9, 5], [(0, 1)] * 3),
        _bar_row("two_bars_tail", [9, 5], [(0, 1)] * 3, tail=7),
        _bar_row("no_bar", [], [(0, 1)] * 3, tail=20),
        _bar_row("empty_bars", [0, 0, 5, 0, 3, 0], [(0, 1), (1, 5), (2, 4)]),
        _bar_row("eos_before_second_bar", [8, 8, 8], [(0, 1), (0, 2), (0, 1)], eos=False, eos_at=25),
        _bar_row("bar_at_255", [60, 60, 60, 59, 20, 20], [(3, 4), (0, 4), (4, 5)]),
        _bar_row("bar_at_256", [60, 60, 60, 60, 20, 20], [(3, 4), (0, 4), (4, 5)]),
        _bar_row("pair_second_out_of_range", [8, 12, 4], [(0, 1), (1, 3), (0, 1)]),
        _bar_row("bar_straddles_256", [60, 60, 60, 54, 11, 30], [(3, 4), (2, 5), (0, 3)]),
        _bar_row("pair_first_negative", [8, 12, 4], [(-1, 2), (0, 1), (0, 1)]),
        _bar_row("two_eos", [8, 12, 4, 6], [(0, 3), (1, 2), (0, 1)], tail=5, eos_at=30),
        _bar_row("pair_unsorted", [8, 12, 4], [(0, 2), (2, 1), (0, 1)]),
        _bar_row("between_flagged", [3, 0, 9, 2], [(0, 3), (0, 1), (1, 3)]),
        _bar_row("pair_equal", [8, 12, 4], [(1, 1), (0, 1), (0, 1)]),
        _bar_row("len4097", [100] * 40 + [43], [(0, 1)] * 3),
        _bar_row("after_oversize", [30, 300, 200, 500], [(0, 3), (1, 2), (0, 2)]),
        _bar_row("empty_prefix", [5, 6, 7], [(0, 2), (0, 1), (1, 2)], prefix=0),
        _many_bars("many_bars_a", [(5, 2047), (2048, 2099), (2047, 2048)]),
        _many_bars("many_bars_b", [(0, 1), (2046, 2049), (2090, 2095)]),
        _bar_row("len4096", [1000, 1000, 1000, 1079], [(0, 3), (1, 2), (0, 2)]),
    ]
    assert [len(r["seq"]) for r in c3 if r["name"] in ("len4097", "len4096")] == [MAX_ROW + 1, MAX_ROW]
    c1 = [_bar_row("c1_ordinary", [8, 12, 4, 16, 8], [(1, 4)]), _bar_row("c1_two_bars", [3, 3], [(0, 1)]),
          _bar_row("c1_seam", [100, 140, 12, 260], [(1, 2)])]
    c0 = [_bar_row("c0_ordinary", [8, 12, 4], []), _bar_row("c0_one_bar", [9], []), _bar_row("c0_seam", [100, 155, 270], [])]
    return [{"name": "count3", "count": 3, "rows": c3}, {"name": "count1", "count": 1, "rows": c1}, {"name": "count0", "count": 0, "rows": c0},
            {"name": "B1", "count": 3, "rows": [_bar_row("single", [8, 12, 4, 16, 8], [(0, 4), (1, 3), (2, 3)])]}]


# ------------------------------------------------------------------------------------------------------------- ragged_to_padded
def r2p_batches():
    out = []
    for L, pad, with_length in ((1, 0, True), (5, 1, True), (255, 0, True), (256, 1, True), (257, 0, False), (257, 1, True)):
        rng = _rng("r2p/%d" % L)
        lens = [min(3, L), 0, L, max(L - 1, 0), L + 3, 1, L + 300]
        rows = [{"name": "L%d_n%d_%d" % (L, n, i), "seq": rng.integers(2, 729, n).astype(I32), "stored": L <= 5} for i, n in enumerate(lens)]
        out.append({"name": "L%d_pad%d%s" % (L, pad, "" if with_length else "_nolength"), "L": L, "pad": pad, "with_length": with_length, "rows": rows})
    out.append({"name": "B1", "L": 40, "pad": 0, "with_length": True, "rows": [{"name": "single", "seq": np.arange(2, 30, dtype=I32), "stored": True}]})
    return out


def r2p_expected(batch):
    """the present behaviour: a row longer than L is truncated and `length` still reports its n (the reference raises there)"""
    L, rows = batch["L"], batch["rows"]
    out = np.full((len(rows), L), batch["pad"], I32)
    for b, r in enumerate(rows):
        k = min(L, len(r["seq"]))
        out[b, :k] = r["seq"][:k]
    return out, np.array([len(r["seq"]) for r in rows], I32)


# ---------------------------------------------------------------------------------------------------------------- meta_to_batch
def m2b_batches():
    out = []
    for B, L, n in ((3, 40, 0), (3, 40, 39), (3, 40, 40), (3, 40, 17), (1, 1, 0), (1, 1, 1), (1, 300, 257), M2B_WRAP + (17,)):
        rng = _rng("m2b/%d/%d/%d" % (B, L, n))
        out.append({"name": "B%d_L%d_n%d" % (B, L, n), "B": B, "L": L, "meta": rng.integers(432, 729, n).astype(I32), "stored": B * L <= 200,
                    "rows": [{"name": "B%d_L%d_n%d" % (B, L, n)}]})
    return out


# --------------------------------------------------------------------------------------------------------------- validate_tokens
def _valid_prefix(rng, k, chords=True):
    """k tokens of valid grammar (BAR | position chord | position velocity pitch duration), starting with a BAR"""
    seq = [2] if k else []
    while len(seq) < k:
        room = k - len(seq)
        if room >= 4 and rng.random() < 0.7:
            seq += [int(rng.integers(432, 560)), int(rng.integers(131, 195)), int(rng.integers(3, 131)), int(rng.integers(304, 432))]
        elif room >= 2 and chords and rng.random() < 0.5:
            seq += [int(rng.integers(432, 560)), int(rng.integers(195, 304))]
        else:
            seq.append(2)
    return seq


def _val_row(name, toks, L, length=None, junk=True):
    rng = _rng("val/" + name)
    row = rng.integers(0, 560, L).astype(I32) if junk else np.zeros(L, I32)
    row[row == 1] = 0
    toks = np.asarray(toks, I32)
    row[:len(toks)] = toks
    return {"name": name, "seq": row, "len": len(toks) if length is None else length, "stored": True}


def val_batches():
    L = 80
    g = _rng("val")
    chord_run = lambda k: [t for _ in range(k) for t in (int(g.integers(432, 560)), int(g.integers(195, 304)))]
    note = [440, 150, 60, 320]
    rows = [
        _val_row("eos0", [1], L), _val_row("eos63", _valid_prefix(g, 63) + [1], L), _val_row("eos64", _valid_prefix(g, 64) + [1], L),
        _val_row("eos65", _valid_prefix(g, 65) + [1], L), _val_row("eos_last", _valid_prefix(g, L - 1) + [1], L),
        _val_row("len0", [], L, 0), _val_row("eos_beyond_len", [2] + note + [1], L, 5), _val_row("eos_at_len_minus_1", [2] + note + [1], L, 6),
        _val_row("no_eos_full", _valid_prefix(g, L), L), _val_row("two_eos", [2] + note + [1] + note + [1], L),
        _val_row("class_0_1_chords_only", [2, 2, 440, 200, 470, 250, 1], L), _val_row("class_0_1_bars_only", [2, 2, 2, 2, 1], L),
        _val_row("class_0_0_garbage", [5, 5, 1], L), _val_row("class_1_0", [2] + note + [7, 1], L), _val_row("class_0_m2", [432, 140, 1], L),
        _val_row("class_0_m2_pitch", [2, 432, 140, 60, 1], L), _val_row("class_1_m2", note + [433, 150, 1], L),
        _val_row("class_1_1", [2] + note + [450, 210] + note + [1], L), _val_row("class_0_0_position_then_eos", [2, 432, 1], L),
        _val_row("once_only_at_63", chord_run(31) + [2] + note + [1], L), _val_row("once_only_at_64", chord_run(31) + [2, 2] + note + [1], L),
        _val_row("once_only_at_65", chord_run(32) + note + [1], L), _val_row("once_needs_position", [2, 150, 60, 320, 1], L),
        _val_row("once_last_slot", [2, 2] + note + [1], L), _val_row("note_cut_by_eos_at_64", chord_run(30) + [2, 440, 150, 60, 1], L),
        _val_row("velocity_first_wraps", [150, 60, 320, 440, 1], L),
    ]
    full = [dict(r, name="nolens_" + r["name"], len=L) for r in rows if r["name"] not in ("len0", "eos_beyond_len")]
    return [{"name": "lens", "L": L, "use_lens": True, "rows": rows}, {"name": "lens_none", "L": L, "use_lens": False, "rows": full},
            {"name": "B1", "L": 7, "use_lens": True, "rows": [_val_row("single", [2] + note + [1], 7)]},
            {"name": "L1", "L": 1, "use_lens": False, "rows": [_val_row("L1_eos", [1], 1), dict(_val_row("L1_bar", [2], 1))]}]


# ----------------------------------------------------------------------------------------------------------------- msim_vectors
def _msim_row(name, toks, L, length=None, status=0, junk=False):
    r = _val_row("msim/" + name, toks, L, length, junk)
    r.update(name=name, status=status)
    return r


def _music(rng, bars, per_bar, chords=0.15, dup=0.3):
    seq = [int(t) for t in rng.integers(3, 131, int(rng.integers(0, 3)))]          # anything may precede the first BAR
    for _ in range(bars):
        seq.append(2)
        pos = sorted(rng.integers(432, 560, per_bar))
        for i, p in enumerate(pos):
            if i and rng.random() < dup:
                p = pos[i - 1]                                                      # two events on one tick (the melody rule)
            if rng.random() < chords:
                seq += [int(p), int(rng.integers(195, 304))]
            else:
                seq += [int(p), int(rng.integers(131, 195)), int(rng.integers(3, 131)), int(rng.integers(304, 432))]
    return seq + [1]


def msim_batches():
    L = 96
    note = [440, 150, 60, 320]
    special = [
        _msim_row("no_bar", note + [1], L, status=1), _msim_row("no_bar_empty", [], L, 0, status=1),
        _msim_row("position_then_garbage", [2, 432, 7, 7, 1], L, status=2), _msim_row("not_a_position", [2, 300, 1], L, status=2),
        _msim_row("off_end_mid_note", [2] + note + [450, 160, 70], L, status=2), _msim_row("off_end_after_position", [2] + note + [450], L, status=2),
        _msim_row("off_end_no_eos", [2] + note + note, L, status=2), _msim_row("bar_last", [5, 2], L, status=2),
        _msim_row("chord_only", [2, 440, 200, 470, 250, 2, 432, 195, 1], L), _msim_row("bar_then_eos", [2, 1], L),
        _msim_row("past_tick_128", [2, 559, 194, 130, 431, 500, 131, 3, 431, 432, 160, 64, 431, 1], L),
        _msim_row("same_start", [2, 440, 150, 60, 320, 440, 140, 72, 310, 440, 130 + 1, 50, 304, 470, 160, 65, 330, 470, 170, 64, 330, 1], L),
        _msim_row("len_shorter_than_row", [2] + note + [460, 170, 66, 340, 1, 2, 7, 7], L, 10),
        _msim_row("len_cuts_note", [2] + note + [460, 170, 66, 340, 1], L, 7, status=2),
        _msim_row("pad_terminates", [2] + note + [0, 9, 9], L, 9), _msim_row("bars_only", [2, 2, 2, 1], L),
        _msim_row("melody_wraps", [2, 432, 150, 100, 310, 440, 150, 30, 310, 450, 150, 129, 310, 2, 433, 150, 5, 310, 1], L),
    ]

    def fill(tag, B, first=()):
        rng = _rng("msim/" + tag)
        rows = list(first)
        while len(rows) < B:
            toks = _music(rng, int(rng.integers(1, 5)), int(rng.integers(1, 5)))[:L - 1]
            toks = _music(rng, 1, 2) if toks[-1] != 1 or 2 not in toks else toks
            rows.append(_msim_row("%s_%d" % (tag, len(rows)), toks, L))
        return rows
    b65 = fill("b65", 65, special)
    b64 = fill("b64", 64)
    none_rows = [dict(r, len=L) for r in fill("nolens", 5)] + [dict(_msim_row("nolens_runs_off", _valid_prefix(_rng("m"), L, False), L, status=2))]
    return [{"name": "B65", "L": L, "use_lens": True, "note_len": 128.0, "rows": b65},
            {"name": "B64", "L": L, "use_lens": True, "note_len": 128.0, "rows": b64},
            {"name": "B1", "L": L, "use_lens": True, "note_len": 128.0, "rows": fill("b1", 1)},
            {"name": "B1_flagged", "L": L, "use_lens": True, "note_len": 128.0, "rows": [_msim_row("single_no_bar", note + [1], L, status=1)]},
            {"name": "note_len96", "L": L, "use_lens": True, "note_len": 96.0, "rows": fill("nl96", 6, special[8:12])},
            {"name": "note_len20", "L": L, "use_lens": True, "note_len": 20.0, "rows": fill("nl20", 4, special[10:12])},
            {"name": "lens_none", "L": L, "use_lens": False, "note_len": 128.0, "rows": none_rows}]


def msim_status(row):
    """0 ok, 1 no BAR, 2 malformed / ran off the end - what the oracle (and the reference) raise on"""
    midi = row["seq"][:row["len"]]
    if not (midi == 2).any():
        return 1
    try:
        with np.errstate(all="ignore"):
            ob.msim_vectors(midi, ref_unbound=False)
    except (AssertionError, IndexError):
        return 2
    return 0


def msim_expected(row, note_len):
    with np.errstate(all="ignore"):
        return ob.msim_vectors(row["seq"][:row["len"]], note_len, ref_unbound=False)


# ------------------------------------------------------------------------------------------------------- controllability_counts
def _ctrl_row(name, L, at=(), length=None, meta=(631, 140, 180), fill=300, extra=0):
    """a row of `fill` (a chord token: counted by nothing) with the tokens of `at` = {position: token}"""
    rng = _rng("ctrl/" + name)
    seq = np.full(L, fill, I32)
    for j, t in dict(at).items():
        seq[j] = t
    m = np.array(_meta(rng)[:11] + [777] * extra, I32)
    m[3], m[7], m[8] = meta[0], meta[1] + 524, meta[2] + 524
    return {"name": name, "seq": seq, "len": L if length is None else length, "meta": m, "stored": L <= STORE_MAX}


def ctrl_counts(row):
    """(pitch sum, pitch count, velocity tokens, those outside [lo, hi]) of one row, the plain way"""
    t = row["seq"][:row["len"]].astype(np.int64)
    lo, hi = int(row["meta"][7]) - 524, int(row["meta"][8]) - 524
    pitch, vel = t[(t >= 3) & (t <= 130)], t[(t >= 131) & (t <= 194)]
    bad = sum(1 for e in vel if not ((lo == 130 or lo <= e) and (hi == 195 or e <= hi)))
    return np.array([pitch.sum(), len(pitch), len(vel), bad], I32)


def ctrl_batches():
    L = 80
    rows = [_ctrl_row("tok%d_at%d" % (t, j), L, {j: t}) for t in (2, 3, 130, 131, 194, 195) for j in (63, 64, 65)]
    rows += [
        _ctrl_row("no_pitch", L, {5: 150, 64: 170, 70: 2}), _ctrl_row("len0", L, {0: 60, 1: 150}, 0),
        _ctrl_row("beyond_len", L, {3: 60, 4: 150, 64: 61, 65: 190}, 64), _ctrl_row("lo_open", L, {1: 131, 64: 194, 65: 181}, meta=(633, 130, 180)),
        _ctrl_row("hi_open", L, {1: 131, 64: 194, 65: 140}, meta=(633, 140, 195)), _ctrl_row("both_open", L, {1: 131, 64: 194}, meta=(630, 130, 195)),
        _ctrl_row("hi_any", L, {1: 131, 64: 194}, meta=(634, 140, 130)), _ctrl_row("bounds_inclusive", L, {1: 140, 2: 180, 3: 139, 64: 181}),
    ]
    rng = _rng("ctrl/random")
    for i in range(6):
        r = _ctrl_row("random_%d" % i, L, meta=(631 + i, 135 + i, 150 + 5 * i))
        r["seq"] = rng.integers(0, 729, L).astype(I32)
        rows.append(r)
    wide = [dict(_ctrl_row("ld13_" + r["name"], L, extra=2), seq=r["seq"], len=r["len"]) for r in rows[:6] + rows[-3:]]
    for w, r in zip(wide, rows[:6] + rows[-3:]):
        w["meta"][:11] = r["meta"]
    big = _ctrl_row("len4096", MAX_ROW, meta=(637, 150, 170))
    big["seq"] = _rng("ctrl/big").integers(0, 729, MAX_ROW).astype(I32)
    big2 = _ctrl_row("len4096_all_pitch", MAX_ROW, fill=130, meta=(637, 150, 170))
    return [{"name": "L80", "L": L, "meta_ld": 11, "use_lens": True, "rows": rows},
            {"name": "meta_ld13", "L": L, "meta_ld": 13, "use_lens": True, "rows": wide},
            {"name": "lens_none", "L": L, "meta_ld": 11, "use_lens": False, "rows": [dict(r, name="nolens_" + r["name"], len=L) for r in rows[:18] + rows[-6:]]},
            {"name": "L4096", "L": MAX_ROW, "meta_ld": 11, "use_lens": True, "rows": [big, big2]},
            {"name": "B1", "L": 65, "meta_ld": 11, "use_lens": True, "rows": [_ctrl_row("single", 65, {0: 3, 64: 131})]}]


# --------------------------------------------------------------------------------------------------------------------- the list
_CACHE = {}


def families():
    """family -> its batches, built once"""
    if not _CACHE:
        note = note_batches()
        _CACHE.update(mt=mt_batches(), mn=note, rn=note, rr=rr_batches(), r2p=r2p_batches(), m2b=m2b_batches(), val=val_batches(),
                      msim=msim_batches(), ctrl=ctrl_batches())
    return _CACHE


def stored_rows(family):
    """(batch, row) of every row the reference runs on, in list order - the fixture's row order"""
    return [(b, r) for b in families()[family] for r in b["rows"] if r.get("stored", b.get("stored", False))]


def oracle_row(family, batch, row):
    """what oracle/batch.py says of one corruption row (raises what the oracle raises)"""
    p = F32(batch.get("p", 0))
    if family == "mt":
        return ob.masking_token(row["seq"], row["u"], p)
    if family == "mn":
        return ob.masking_note(row["seq"], row["u"], p)
    if family == "rn":
        return ob.randomize_note(row["seq"], row["u"], row["new"], p)
    if family == "rr":
        return ob.random_rotating(row["seq"], row["pairs"])
    raise KeyError(family)
