"""Edge matrix of the batch, validator and metric kernels (csrc/batch.hip): every C entry point called through the library's ABI on every
row of the shared case list (tests/batch_cases.py) - chunk seams (tokens 255 / 256 / 257, 511..513, 4095 / 4096), the single-wave strides
(63 / 64 / 65), empty rows, B = 1, rows without EOS or with several, a 4097-token row, 2100 bars in one row, the second sweep of
meta_to_batch's grid-stride loop, MSIM batches of 1 / 64 / 65 - EVERY row and EVERY element compared, none sampled.

Expected values: what the reference itself returned on the row where tests/golden/batch_edges.npz holds it (the short rows), else
oracle/batch.py on the generated row (tests/test_batch_cases_cpu.py holds the oracle to the reference, exceptions included).  Integer
outputs bit for bit.  MSIM vectors rtol 3e-6, atol 3e-7, the tolerance tests/test_batch_gpu.py uses against the oracle (fp32 norms summed
in another order); NaN (the 0 / 0 harmony of a row without notes) must sit exactly where the expectation has it.  No case needed more:
the worst |got - ref| / (atol + rtol |ref|) measured on an MI355X over all MSIM cases is 0.057 (every case prints its own
BATCH-MATRIX msim line), note_len 96 and 20 included.

Every output and status buffer is SLACK elements larger on both sides than the documented output and starts filled with a value no kernel
produces (int32: a large negative number; float: a NaN with a payload no arithmetic yields); everything outside the documented output
must still hold it afterwards, and nothing inside may.

Pinned where the kernels deliberately differ from the reference (documented in data/corruption.py, data/wrapper.py, metric.py):
random_rotating flags rows instead of raising or changing their length; ragged_to_padded truncates a row longer than L and still
reports its length; a row with no position token before its EOS ([2, 1]) gets flat MSIM vectors and status 0 where the reference raises
UnboundLocalError; Controllability_Pitch clamps a range token outside 631..637 to the nearest range where the reference raises KeyError."""
import numpy as np
import pytest
import torch

import batch_cases as bc
from conftest import load_golden

pytestmark = pytest.mark.gpu

from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import check, current_stream, lib  # noqa: E402
from oracle import batch as ob  # noqa: E402

DEV = "cuda"
SLACK = 256
SENT = -(2 ** 31) + 12345                  # int32 outputs are tokens, lengths, counts and small statuses: none is this
NAN_BITS = 0x7FC12345                      # a quiet NaN with a payload; 0 / 0 gives 0x7FC00000 or 0xFFC00000
I32, F32 = np.int32, np.float32
FAM = bc.families()
ids = lambda b: b["name"]


@pytest.fixture(scope="module")
def g():
    z = load_golden("batch_edges.npz")
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def index(g):
    return {fam: {n: i for i, n in enumerate(g[fam + "_names"])} for fam in FAM}


# ------------------------------------------------------------------------------------------------------------------ buffers
def dev(a, dtype=I32):
    """an input on the device; one spare element, so that an empty input still has an address"""
    a = np.ascontiguousarray(a, dtype).ravel()
    return torch.from_numpy(np.concatenate([a, np.zeros(1, dtype)])).to(DEV)


class Guarded:
    """an output of n int32 / float32 elements with SLACK sentinel elements in front of it and behind it"""

    def __init__(self, n, what, floats=False):
        self.n, self.what, self.floats = int(n), what, floats
        self.t = torch.full((self.n + 2 * SLACK,), NAN_BITS if floats else SENT, dtype=torch.int32, device=DEV)
        self.fill = NAN_BITS if floats else SENT

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * SLACK

    def read(self, written=None):
        """the documented output; the guard bands must be untouched, and (written: mask or None = all) every element written"""
        a = self.t.cpu().numpy()
        assert (a[:SLACK] == self.fill).all() and (a[SLACK + self.n:] == self.fill).all(), "%s: written outside its %d elements" % (self.what, self.n)
        body = a[SLACK:SLACK + self.n]
        untouched = body == self.fill
        if written is None:
            assert not untouched.any(), "%s: %d elements never written, first %d" % (self.what, int(untouched.sum()), int(np.argmax(untouched)))
        else:
            assert np.array_equal(~untouched, np.asarray(written).ravel()), "%s: wrote other elements than documented" % self.what
        return body.view(F32) if self.floats else body


def run(fn, *args):
    """args: device tensors and Guarded outputs are passed by address and stay referenced until the kernel has finished (a temporary
    freed before the launch would hand its block to the next input)"""
    raw = [a.data_ptr() if torch.is_tensor(a) else a.ptr if isinstance(a, Guarded) else a for a in args]
    check(fn(*raw, current_stream()), fn.__name__)
    torch.cuda.synchronize()


def expected(g, index, fam, batch, row):
    """the reference's own output where the fixture holds one for this row, else the oracle's"""
    i = index[fam].get("%s/%s" % (batch["name"], row["name"]))
    if i is not None and g[fam + "_exc"][i] == 0:
        o = g[fam + "_out_offsets"]
        assert np.array_equal(g[fam + "_values"][g[fam + "_offsets"][i]:g[fam + "_offsets"][i + 1]], row["seq"])
        return g[fam + "_out"][o[i]:o[i + 1]]
    return bc.oracle_row(fam, batch, row)


def compare_rows(fam, batch, got, off, exp_of):
    for b, r in enumerate(batch["rows"]):
        exp = exp_of(r)
        a = got[off[b]:off[b + 1]]
        assert np.array_equal(a, exp), "%s %s/%s: %d of %d tokens differ, first at %d" % (
            fam, batch["name"], r["name"], int((a != exp).sum()), len(exp), int(np.argmax(a != exp)))


# -------------------------------------------------------------------------------------------------------------- corruptions
@pytest.mark.parametrize("batch", FAM["mt"], ids=ids)
def test_masking_token(batch, g, index):
    rows = batch["rows"]
    vals, off = bc.ragged(rows)
    u, _ = bc.ragged(rows, "u", F32)
    out = Guarded(len(vals), "masking_token out")
    run(lib().mh_corrupt_masking_token, dev(vals), dev(off, np.int64), dev(u, F32), float(batch["p"]), out, len(rows))
    compare_rows("mt", batch, out.read(), off, lambda r: expected(g, index, "mt", batch, r))


@pytest.mark.parametrize("mode", ["mn", "rn"])
@pytest.mark.parametrize("batch", FAM["mn"], ids=ids)
def test_masking_note_and_randomize_note(batch, mode, g, index):
    rows = batch["rows"]
    vals, off = bc.ragged(rows)
    u, _ = bc.ragged(rows, "u", F32)
    new, _ = bc.ragged(rows, "new", I32, 3)
    out = Guarded(len(vals), mode + " out")
    v, o, ud = dev(vals), dev(off, np.int64), dev(u, F32)
    if mode == "mn":
        run(lib().mh_corrupt_masking_note, v, o, ud, float(batch["p"]), out, len(rows))
    else:
        nd = dev(new)
        run(lib().mh_corrupt_randomize_note, v, o, ud, nd, float(batch["p"]), out, len(rows))
    compare_rows(mode, batch, out.read(), off, lambda r: expected(g, index, mode, batch, r))


def oversize_row():
    return next(r for r in FAM["rr"][0]["rows"] if r["name"] == "len4097")


@pytest.mark.parametrize("mode", ["mn", "rn"])
def test_note_kernels_pass_an_oversize_row_through(mode):
    """the wrappers reject a 4097-token row; handed straight to the C ABI the kernels copy it through (they index LDS by token) and
    still corrupt its neighbours"""
    big = oversize_row()["seq"].copy()
    big[::5] = 150                                                   # velocity tokens that would all fire
    left, right = FAM["mn"][0]["rows"][0], FAM["mn"][0]["rows"][3]   # vel0, n3_vel0_fires
    n = len(big)
    mk = lambda seq: {"seq": seq, "u": np.full(len(seq), 0.25, F32), "new": np.tile(np.array([140, 60, 320], I32), (len(seq), 1))}
    rows = [left, mk(big), right]
    vals, off = bc.ragged(rows)
    u, _ = bc.ragged(rows, "u", F32)
    new, _ = bc.ragged(rows, "new", I32, 3)
    out = Guarded(len(vals), mode + " oversize out")
    v, o, ud, nd = dev(vals), dev(off, np.int64), dev(u, F32), dev(new)
    if mode == "mn":
        run(lib().mh_corrupt_masking_note, v, o, ud, 0.5, out, 3)
    else:
        run(lib().mh_corrupt_randomize_note, v, o, ud, nd, 0.5, out, 3)
    got = out.read()
    assert n == bc.MAX_ROW + 1 and np.array_equal(got[off[1]:off[2]], big)
    for b in (0, 2):
        assert np.array_equal(got[off[b]:off[b + 1]], bc.oracle_row(mode, {"p": 0.5}, rows[b]))


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "status_null"])
@pytest.mark.parametrize("batch", FAM["rr"], ids=ids)
def test_random_rotating(batch, with_status, g, index):
    rows, count = batch["rows"], batch["count"]
    vals, off = bc.ragged(rows)
    pairs = np.stack([r["pairs"] for r in rows]).reshape(len(rows), count, 2)
    out, status = Guarded(len(vals), "random_rotating out"), Guarded(len(rows), "random_rotating status")
    run(lib().mh_corrupt_random_rotating, dev(vals), dev(off, np.int64), dev(pairs), count, out,
        status if with_status else None, len(rows))
    got = out.read()
    st = status.read(None if with_status else np.zeros(len(rows), bool))
    for b, r in enumerate(rows):
        a = got[off[b]:off[b + 1]]
        what = "rr %s/%s" % (batch["name"], r["name"])
        if with_status:
            assert st[b] == r["status"], (what, int(st[b]))
        if r["status"] == 0:
            exp = expected(g, index, "rr", batch, r)
            assert np.array_equal(a, exp), "%s: %d tokens differ, first at %d" % (what, int((a != exp).sum()), int(np.argmax(a != exp)))
        elif r["status"] == 2:
            assert np.array_equal(a, r["seq"]), what                                        # passed through
        else:
            assert np.array_equal(np.sort(a), np.sort(r["seq"])), what                      # its length (by layout) and its multiset of tokens
    assert {r["status"] for r in rows} >= ({0, 1, 2} if batch["name"] == "count3" else {0})


# ---------------------------------------------------------------------------------------------- ragged_to_padded, meta_to_batch
@pytest.mark.parametrize("batch", FAM["r2p"], ids=ids)
def test_ragged_to_padded(batch):
    rows, L = batch["rows"], batch["L"]
    vals, off = bc.ragged(rows)
    out, length = Guarded(len(rows) * L, "ragged_to_padded out"), Guarded(len(rows), "ragged_to_padded length")
    run(lib().mh_ragged_to_padded, dev(vals), dev(off, np.int64), out, length if batch["with_length"] else None,
        len(rows), L, batch["pad"])
    exp, exp_len = bc.r2p_expected(batch)
    assert np.array_equal(out.read().reshape(len(rows), L), exp)
    got_len = length.read(None if batch["with_length"] else np.zeros(len(rows), bool))
    if batch["with_length"]:
        assert np.array_equal(got_len, exp_len)                      # a truncated row still reports its own n


@pytest.mark.parametrize("batch", FAM["m2b"], ids=ids)
def test_meta_to_batch(batch):
    B, L, meta = batch["B"], batch["L"], batch["meta"]
    i, m = Guarded(B * L, "meta_to_batch ids"), Guarded(B * L, "meta_to_batch mask")
    run(lib().mh_meta_to_batch, dev(meta), len(meta), i, m, B, L)
    ei, em = ob.meta_to_batch(meta, B, L)
    assert np.array_equal(i.read().reshape(B, L), ei) and np.array_equal(m.read().reshape(B, L), em)


# ----------------------------------------------------------------------------------------------------------------- validators
def table(batch):
    rows = batch["rows"]
    toks = np.stack([r["seq"] for r in rows]).astype(I32)
    lens = np.array([r["len"] for r in rows], I32)
    assert toks.shape == (len(rows), batch["L"]) and (batch["use_lens"] or (lens == batch["L"]).all())
    return toks, lens


@pytest.mark.parametrize("batch", FAM["val"], ids=ids)
def test_validate_tokens(batch, g, index):
    toks, lens = table(batch)
    B, L = toks.shape
    res = Guarded(B * 3, "validate_tokens result")
    ld = dev(lens)
    run(lib().mh_validate_tokens, dev(toks), ld if batch["use_lens"] else None, res, B, L)
    got = res.read().reshape(B, 3)
    for b, r in enumerate(batch["rows"]):
        i = index["val"]["%s/%s" % (batch["name"], r["name"])]
        assert tuple(got[b]) == tuple(g["val_result"][i]) == ob.validate(r["seq"], r["len"]), (batch["name"], r["name"], got[b], g["val_result"][i])


# ---------------------------------------------------------------------------------------------------------------------- metric
RTOL, ATOL = 3e-6, 3e-7


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "status_null"])
@pytest.mark.parametrize("batch", FAM["msim"], ids=ids)
def test_msim_vectors(batch, with_status, g, index):
    toks, lens = table(batch)
    B, L = toks.shape
    out, status = Guarded(B * 56, "msim_vectors out", floats=True), Guarded(B, "msim_vectors status")
    ld = dev(lens)
    run(lib().mh_msim_vectors, dev(toks), ld if batch["use_lens"] else None, out, status if with_status else None,
        B, L, float(batch["note_len"]))
    got = out.read().reshape(B, 56)
    st = status.read(None if with_status else np.zeros(B, bool))
    worst = 0.0
    for b, r in enumerate(batch["rows"]):
        what = "msim %s/%s" % (batch["name"], r["name"])
        if with_status:
            assert st[b] == r["status"], (what, int(st[b]))
        if r["status"] != 0:
            continue                                                 # a flagged row's vectors are not part of the contract
        i = index["msim"].get("%s/%s" % (batch["name"], r["name"]))
        ref = g["msim_vectors"][i] if i is not None and g["msim_exc"][i] == 0 else bc.msim_expected(r, batch["note_len"])
        assert np.array_equal(np.isnan(got[b]), np.isnan(ref)), what  # NaN exactly where the expectation has it
        ok = ~np.isnan(ref)
        err = np.abs(got[b][ok].astype(np.float64) - ref[ok]) / (ATOL + RTOL * np.abs(ref[ok].astype(np.float64)))
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, "%s: element %d off by %.3g of its tolerance (got %.9g, ref %.9g)" % (
            what, int(np.argmax(err)), err.max(), got[b][ok][np.argmax(err)], ref[ok][np.argmax(err)])
    print("BATCH-MATRIX msim %s worst err / tol %.3f" % (batch["name"], worst))


@pytest.mark.parametrize("batch", FAM["ctrl"], ids=ids)
def test_controllability_counts(batch):
    toks, lens = table(batch)
    B, L = toks.shape
    ld_m = batch["meta_ld"]
    metas = np.stack([r["meta"] for r in batch["rows"]]).astype(I32)
    assert metas.shape == (B, ld_m)
    out = Guarded(B * 4, "controllability_counts out")
    ld = dev(lens)
    run(lib().mh_controllability_counts, dev(toks), ld if batch["use_lens"] else None, dev(metas), ld_m, out, B, L)
    got = out.read().reshape(B, 4)
    for b, r in enumerate(batch["rows"]):
        assert np.array_equal(got[b], bc.ctrl_counts(r)), (batch["name"], r["name"], got[b], bc.ctrl_counts(r))


def test_controllability_wrappers_on_the_edge_rows():
    """the host half (mean, range lookup, the sums) on the rows whose counts the kernel test pins: a row without pitch tokens counts as
    wrong, as the reference's NaN mean does; and the pinned clamp of a range token outside 631..637"""
    from musediffusion_amd import metric as mm
    batch = FAM["ctrl"][0]
    toks, lens = table(batch)
    metas = np.stack([r["meta"] for r in batch["rows"]]).astype(I32)
    t, l, m = (torch.from_numpy(a).to(DEV) for a in (toks, lens, metas))
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            (pt, pw), (vt, vw) = ob.controllability(metas, [r["seq"][:r["len"]] for r in batch["rows"]])
    assert tuple(mm.Controllability_Pitch(m, t, l)) == (pt, pw) and tuple(mm.Controllability_Velocity(m, t, l)) == (vt, vw)
    assert pw > 0 and 0 < vw < vt
    one = [r["name"] for r in batch["rows"]].index("no_pitch")
    assert mm.Controllability_Pitch(m[one:one + 1], t[one:one + 1], l[one:one + 1]) == (1, 1)
    # range tokens 629 / 640 (the reference: KeyError) are judged by the ranges of 631 / 637
    row = torch.full((2, 8), 300, dtype=torch.int32, device=DEV)
    row[0, 0], row[1, 0] = 20, 120
    for lo_tok, hi_tok, want in ((629, 640, 0), (640, 629, 2)):
        mt = m[:2].clone()
        mt[0, 3], mt[1, 3] = lo_tok, hi_tok
        assert mm.Controllability_Pitch(mt, row) == (2, want)


# ------------------------------------------------------------------------------------------------------- wrappers and bad arguments
def test_row_limit_and_the_wrappers_own_checks():
    from musediffusion_amd import data as mdata
    assert lib().mh_batch_max_row() == bc.MAX_ROW
    rng = np.random.default_rng(0)
    at_limit = np.where(rng.random(bc.MAX_ROW) < 0.2, 150, 440).astype(I32)
    v, off = mdata.to_ragged([at_limit, at_limit[:50]], DEV)
    assert mdata.masking_note(v, off, 0.5).shape == v.shape                                 # 4096 tokens: accepted
    v, off = mdata.to_ragged([at_limit[:50], np.concatenate([at_limit, [1]])], DEV)         # 4097: rejected before any launch
    for fn in (mdata.masking_note, mdata.randomize_note, mdata.random_rotating):
        with pytest.raises(ValueError, match="4097 tokens exceeds the 4096-token row limit"):
            fn(v, off)
    # collate_batches truncates a row longer than seq_len and reports its own length (the reference raises there)
    col = mdata.collate_batches({"input_ids": v, "input_mask": torch.ones_like(v)}, off, 60)
    assert col["length"].tolist() == [50, 4097] and torch.equal(col["input_ids"][1].cpu(), torch.from_numpy(at_limit[:60]))
    assert col["input_mask"][0].tolist() == [1] * 60 and col["input_ids"][0, 50:].tolist() == [0] * 10


def test_bad_arguments_are_rejected_not_launched():
    L = lib()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    off = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = Guarded(64, "rejected call")
    p, o, s = buf.data_ptr(), off.data_ptr(), current_stream()
    calls = [
        (L.mh_ragged_to_padded, (None, o, out.ptr, None, 1, 8, 0)), (L.mh_ragged_to_padded, (p, o, out.ptr, None, 0, 8, 0)),
        (L.mh_ragged_to_padded, (p, o, out.ptr, None, 1, 0, 0)), (L.mh_ragged_to_padded, (p, o, None, None, 1, 8, 0)),
        (L.mh_meta_to_batch, (p, 9, out.ptr, out.ptr, 1, 8)), (L.mh_meta_to_batch, (p, -1, out.ptr, out.ptr, 1, 8)),
        (L.mh_meta_to_batch, (p, 1, out.ptr, None, 1, 8)), (L.mh_meta_to_batch, (p, 1, out.ptr, out.ptr, 0, 8)),
        (L.mh_corrupt_masking_token, (p, o, None, 0.3, out.ptr, 1)), (L.mh_corrupt_masking_token, (p, o, p, 0.3, out.ptr, 0)),
        (L.mh_corrupt_masking_note, (p, None, p, 0.5, out.ptr, 1)), (L.mh_corrupt_masking_note, (p, o, p, 0.5, None, 1)),
        (L.mh_corrupt_randomize_note, (p, o, p, None, 0.5, out.ptr, 1)), (L.mh_corrupt_randomize_note, (p, o, p, p, 0.5, out.ptr, -1)),
        (L.mh_corrupt_random_rotating, (p, o, p, -1, out.ptr, None, 1)), (L.mh_corrupt_random_rotating, (p, o, None, 1, out.ptr, None, 1)),
        (L.mh_validate_tokens, (p, None, None, 1, 8)), (L.mh_validate_tokens, (p, None, out.ptr, 1, 0)),
        (L.mh_msim_vectors, (p, None, out.ptr, None, 1, 8, 0.0)), (L.mh_msim_vectors, (None, None, out.ptr, None, 1, 8, 128.0)),
        (L.mh_controllability_counts, (p, None, p, 8, out.ptr, 1, 8)), (L.mh_controllability_counts, (p, None, None, 11, out.ptr, 1, 8)),
    ]
    for fn, args in calls:
        assert fn(*args, s) == _lib.MH_ERR_INVALID, (fn.__name__, args)
        with pytest.raises(_lib.MuseHipError, match="bad arguments"):
            check(fn(*args, s), fn.__name__)
    torch.cuda.synchronize()
    out.read(np.zeros(64, bool))
