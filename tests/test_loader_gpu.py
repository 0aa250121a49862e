"""GPU: csrc/loader.hip through the C ABI against the numpy restatement (tests/loader_ref.py, itself pinned to the reference's
recorded answers by tests/test_loader_cpu.py), then the Python surface - augment_rows, per-sequence Corruptions, MusicDataset,
load_data_music - against the fixture tests/golden/loader.npz.  Integer work: every comparison is exact.  Outputs start filled with
a sentinel and carry a guard band behind them that must come back untouched; indices out of range, capacities one short and hostile
rows are legal input that must end in a status - no test here tries to provoke a fault."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loader_ref as lr  # noqa: E402
from gpu_helpers import library_launches  # noqa: E402
from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd import data as mdata  # noqa: E402
from musediffusion_amd.data import dataset as mds  # noqa: E402
from musediffusion_amd.utils import encode_util as menc  # noqa: E402
from test_encode_gpu import SENTINEL, check_guards, dev, guarded  # noqa: E402
from test_loader_cpu import corruption_draws, d_cases, d_rows, fixture, rag, write_pair  # noqa: E402

DEV = "cuda"
STREAM = _lib.current_stream


def source(seed=0, extra=()):
    """a ragged source: rows of length 0, 1 and exactly 4096 among random ones -> (values, offsets, rows)"""
    g = np.random.default_rng(seed)
    lens = [0, 1, 4096, 17, 300, 0, 255, 256, 257, 1024, 5] + list(extra)
    rows = [g.integers(0, 729, n).astype(np.int32) for n in lens]
    values, offsets = lr.ragged(rows)
    return values, offsets, rows


def run_gather(values, offsets, idx, cap, second=None):
    """mhd_gather_offsets + mhd_gather_rows per field through the C ABI, guarded -> dict of numpy arrays"""
    B, n = len(idx), len(offsets) - 1
    v, o, i = dev(values), dev(offsets, np.int64), dev(idx, np.int64)
    bufs = {k: guarded(s, t) for k, s, t in (("offsets", (B + 1,), torch.int64), ("length", (B,), torch.int32), ("status", (B,), torch.int32),
                                             ("out", (max(cap, 1),), torch.int32), ("out2", (max(cap, 1),), torch.int32))}
    w = {k: b[1] for k, b in bufs.items()}
    L = _lib.lib()
    _lib.check(L.mhd_gather_offsets(o.data_ptr(), n, i.data_ptr(), w["offsets"].data_ptr(), w["length"].data_ptr(), w["status"].data_ptr(),
                                    B, cap, STREAM()), "mhd_gather_offsets")
    _lib.check(L.mhd_gather_rows(v.data_ptr(), o.data_ptr(), n, i.data_ptr(), w["offsets"].data_ptr(), w["length"].data_ptr(),
                                 w["out"].data_ptr(), B, cap, STREAM()), "mhd_gather_rows")
    if second is not None:                                                # a second field shares the offsets
        s = dev(second)
        _lib.check(L.mhd_gather_rows(s.data_ptr(), o.data_ptr(), n, i.data_ptr(), w["offsets"].data_ptr(), w["length"].data_ptr(),
                                     w["out2"].data_ptr(), B, cap, STREAM()), "mhd_gather_rows")
    torch.cuda.synchronize()
    check_guards(bufs)
    return {k: x.cpu().numpy() for k, x in w.items()}


def check_gather(values, offsets, idx, cap, second=None):
    got = run_gather(values, offsets, idx, cap, second)
    off, length, status = lr.gather_offsets(offsets, idx, cap)
    assert np.array_equal(got["offsets"], off) and np.array_equal(got["length"], length) and np.array_equal(got["status"], status)
    want = lr.gather_rows(values, offsets, idx, off, length, np.full(max(cap, 1), SENTINEL, np.int32))
    assert np.array_equal(got["out"], want)
    if second is not None:
        assert np.array_equal(got["out2"], lr.gather_rows(second, offsets, idx, off, length, np.full(max(cap, 1), SENTINEL, np.int32)))
    return got, status


def test_gather_through_the_c_abi():
    values, offsets, rows = source()
    n = len(rows)
    second = (values + 1000).astype(np.int32)
    g = np.random.default_rng(1)
    for B in (1, 7, 64):
        idx = g.integers(0, n, B)
        idx[0] = 2                                                        # the 4096-token row
        check_gather(values, offsets, idx, B * 4096, second)
    check_gather(values, offsets, [4, 4, 4, 3, 3], 5 * 4096)              # repeated
    check_gather(values, offsets, list(range(n - 1, -1, -1)), n * 4096)   # descending, with the rows of length 0, 1 and 4096
    check_gather(values, offsets, [0, 5, 0], 1)                           # empty rows only
    _, st = check_gather(values, offsets, [3, -1, 4, n, 1, 2 ** 40, -2 ** 40], 7 * 4096)   # an index of -1 and one of n: empty rows
    assert st.tolist() == [0, 1, 0, 1, 0, 1, 1]
    idx = [4, 3, 1, 9, 0, 6]
    total = int(sum(len(rows[i]) for i in idx))
    _, st = check_gather(values, offsets, idx, total)                     # exactly enough
    assert not st.any()
    got, st = check_gather(values, offsets, idx, total - 1)               # one token short: the last non-empty row is cut
    assert st.tolist() == [0, 0, 0, 0, 0, 2] and got["length"][5] == 0 and got["offsets"][-1] == total - len(rows[6])
    _, st = check_gather(values, offsets, idx, len(rows[4]) + len(rows[3]))   # everything behind the cut goes, empty rows keep OK
    assert st.tolist() == [0, 0, 2, 2, 0, 2]
    # more than one pass of the 256-thread scan, with a cut in the middle of a later pass
    big = g.integers(0, n, 1000)
    check_gather(values, offsets, big, 1000 * 4096)
    part = int(sum(len(rows[i]) for i in big[:700]))
    _, st = check_gather(values, offsets, big, part)
    assert not st[:700].any() and (st[700:] == 2).any()


def run_select(a, b, offsets, take, alias):
    B = len(offsets) - 1
    bufs = {"out": guarded((len(a),))}
    out = bufs["out"][1]
    av = out if alias else dev(a)
    if alias:
        out.copy_(dev(a))
    bv, o, t = dev(b), dev(offsets, np.int64), dev(take)
    _lib.check(_lib.lib().mhd_select_rows(av.data_ptr(), bv.data_ptr(), o.data_ptr(), t.data_ptr(), out.data_ptr(), B, STREAM()), "mhd_select_rows")
    torch.cuda.synchronize()
    check_guards(bufs)
    return out.cpu().numpy()


def test_select_through_the_c_abi():
    values, offsets, rows = source(2)
    other = (values + 2000).astype(np.int32)
    g = np.random.default_rng(3)
    for take in (g.integers(0, 2, len(rows)), np.zeros(len(rows), np.int64), np.full(len(rows), 7), g.integers(-1, 2, len(rows))):
        want = lr.select_rows(values, other, offsets, take)
        for alias in (False, True):
            assert np.array_equal(run_select(values, other, offsets, take.astype(np.int32), alias), want)


def run_augment(values, offsets, key, bpm, alias=False):
    B = len(offsets) - 1
    bufs = {"out": guarded((max(len(values), 1),)), "status": guarded((B,))}
    w = {k: b[1] for k, b in bufs.items()}
    o, kc, bc = dev(offsets, np.int64), dev(key), dev(bpm)
    v = w["out"] if alias else dev(values)
    if alias:
        w["out"][:len(values)].copy_(dev(values))
    _lib.check(_lib.lib().mhd_augment_rows(v.data_ptr(), o.data_ptr(), kc.data_ptr(), bc.data_ptr(), w["out"].data_ptr(), w["status"].data_ptr(),
                                           B, STREAM()), "mhd_augment_rows")
    torch.cuda.synchronize()
    check_guards(bufs)
    return w["out"].cpu().numpy()[:len(values)], w["status"].cpu().numpy()


def check_augment(rows, key, bpm):
    values, offsets = lr.ragged(rows)
    want, status = lr.augment_rows(values, offsets, key, bpm)
    for alias in (False, True):
        got, st = run_augment(values, offsets, key, bpm, alias)
        assert np.array_equal(st, status) and np.array_equal(got, want)
    return status


ROW = np.array([580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727, 432, 195, 448, 302, 1, 2, 432, 150, 60, 320, 440, 303, 470, 131, 9,
                304, 480, 194, 124, 431, 1], np.int32)


def test_augment_through_the_c_abi():
    grid = [(k, c) for k in lr.KEY_CHANGES for c in lr.BPM_CHANGES]
    st = check_augment([ROW] * 60, [k for k, _ in grid], [c for _, c in grid])     # every (k, c) of the grid on one row
    assert not st.any()
    minor = ROW.copy()
    minor[0], minor[1] = 561, 623
    assert not check_augment([minor] * 60, [k for k, _ in grid], [c for _, c in grid]).any()
    cases, keys = [], []
    for k in lr.KEY_CHANGES:                                               # the highest pitch one out of range for k > 0, the lowest for k < 0
        r = ROW.copy()
        r[19] = 3 + (127 - k + 1 if k > 0 else -k - 1 if k < 0 else 127)
        cases += [r, r]
        keys += [k, k - 1 if k > 0 else k + 1 if k < 0 else 0]
    st = check_augment(cases, keys, [1] * len(cases))
    assert st.tolist() == [x for k in lr.KEY_CHANGES for x in ((lr.PITCH_RANGE, lr.AUGMENT_OK) if k else (0, 0))]
    other, short, hostile, both = ROW.copy(), ROW[:11], ROW.copy(), ROW.copy()
    other[1] = 614                                                        # cminor: not an origin key
    hostile[2:11] = [60, 200, 3, 130, 195, 302, 303, 64, 250]             # pitch- and chord-valued tokens inside the first 11
    both[1], both[19] = 601, 130                                          # no origin AND a pitch out of range: NOT_ORIGIN is decided first
    g = np.random.default_rng(5)
    long_ok = np.concatenate([ROW[:12], g.integers(9, 125, 4096 - 12).astype(np.int32)])
    too_long = np.concatenate([ROW, np.zeros(4097 - len(ROW), np.int32)])
    noise = g.integers(-5, 740, 700).astype(np.int32)
    noise[1] = 623
    rows = [other, short, hostile, both, long_ok, too_long, noise, ROW[:12], ROW[:0], ROW, ROW, ROW, ROW]
    st = check_augment(rows, [3, 3, -6, 5, 5, 1, -6, 2, 0, 6, -7, 0, 0], [1, 1, 2, 0, -2, 0, 2, 1, 0, 0, 0, 3, -3])
    assert st.tolist() == [lr.NOT_ORIGIN, lr.BAD_ROW, 0, lr.NOT_ORIGIN, 0, lr.BAD_ROW, st[6], 0, lr.BAD_ROW] + [lr.BAD_ROW] * 4
    blocks = [r for _ in range(40) for r in (ROW, minor, long_ok)]       # more rows than one wave of blocks, mixed lengths
    check_augment(blocks, g.integers(-6, 6, len(blocks)), g.integers(-2, 3, len(blocks)))


def test_augment_rows_equals_the_reference_augmentation():
    """the fixture's end-to-end cases: augment_rows(unaugmented row) == the row the reference made from the augmented file"""
    rows = d_rows()
    base = {ci: ids for ci, k, c, st, ids, _ in rows if (k, c) == (0, 0) and st == 0}
    todo = [r for r in rows if r[0] in base]
    values, offsets = lr.ragged([base[r[0]] for r in todo])
    out, status = mdata.augment_rows(dev(values), dev(offsets, np.int64), [r[1] for r in todo], [r[2] for r in todo], return_status=True)
    assert out.is_cuda and out.dtype == torch.int32
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert len(todo) == 190 and status.tolist() == [(lr.AUGMENT_OK, None, lr.PITCH_RANGE)[r[3]] for r in todo]
    for i, (ci, k, c, st, ids, _) in enumerate(todo):
        assert np.array_equal(out[offsets[i]:offsets[i + 1]], ids if st == 0 else base[ci]), (ci, k, c)
    # no draws given: they come from the device generator, on the reference's grid
    torch.manual_seed(5)
    a, sa = mdata.augment_rows(dev(values), dev(offsets, np.int64), return_status=True)
    torch.manual_seed(5)
    b = mdata.Augment()(dev(values), dev(offsets, np.int64))
    sa = sa.cpu().numpy()
    assert torch.equal(a, b) and not torch.equal(a, dev(values)) and set(sa.tolist()) <= {lr.AUGMENT_OK, lr.PITCH_RANGE}
    got = lr.rows_of(a.cpu().numpy(), offsets)
    for i, (ci, *_rest) in enumerate(todo):
        if sa[i] == 0:
            k = (int(got[i][1]) - int(base[ci][1])) % 12
            k = k - 12 if k > 5 else k
            c = int(got[i][0]) - int(base[ci][0])
            assert abs(c) <= 2 and np.array_equal(got[i][2:], lr.augment_row(base[ci], k, 0)[0][2:]), i


def test_closed_loop_on_project_code():
    """encode_notes(moved notes, rotated names) followed by merge_and_mask == augment_rows of the unmoved encoding"""
    cases = [c for c in d_cases() if c["meta"]["audio_key"] in ("cmajor", "aminor") and c["notes"][:, 2].min() >= 6 and c["notes"][:, 2].max() <= 121]
    assert len(cases) >= 15
    m2s = menc.MetaToSequence()

    def encode(k):
        notes = []
        for c in cases:
            n = c["notes"].copy()
            n[:, 2] += k
            notes.append(n)
        params = [(480, 4, 4, int(np.ceil(c["meta"]["num_measures"])), 0) for c in cases]
        enc = menc.encode_notes(*menc.pack_items(notes, params, [[lr.rotate_name(n, k) for n in c["names"]] for c in cases]))
        src = np.array([m2s.encode_meta(c["meta"]) for c in cases], np.int32)
        src[:, 1] = [lr.key_token(int(t), k) for t in src[:, 1]]
        fields, offsets, length, status = menc.merge_and_mask(src, enc.words, enc.lengths, enc.status)
        assert not status.cpu().any()
        return fields["input_ids"], offsets, int(offsets[-1])

    base, offsets, total = encode(0)
    for k in (-6, -1, 3, 5):
        moved, off_k, total_k = encode(k)
        assert torch.equal(off_k, offsets)
        got, status = mdata.augment_rows(base[:total], offsets, [k] * len(cases), [0] * len(cases), return_status=True)
        assert not status.cpu().any() and torch.equal(got, moved[:total_k]), k


def test_per_sequence_corruption_equals_the_reference_row_by_row():
    f = fixture()
    values, offsets = dev(f["b_values"]), dev(f["b_off"], np.int64)
    for c, (corr_max, corr_p) in enumerate(f["b_configs"]):
        d = corruption_draws(c)
        corr = mdata.Corruptions(("mt", "mn", "rn", "rr"), int(corr_max), float(corr_p))
        # u[r, offsets[b] + i]: draw i of row b in slot r, whichever kind fired there - the layout all three functions document
        draws = {(r, key): kw for r in range(int(corr_max)) for key, kw in
                 (("mt", dict(u=torch.from_numpy(d["u"][r]))), ("mn", dict(u=torch.from_numpy(d["u"][r]))),
                  ("rn", dict(u=torch.from_numpy(d["u"][r]), new_tokens=torch.from_numpy(d["new"][r]))),
                  ("rr", dict(pairs=torch.from_numpy(d["pairs"][r]))))}
        before = values.clone()
        got = corr(values, offsets, per_sequence=True, choices=f["b%d_choices" % c], draws=draws)
        assert torch.equal(values, before) and got.data_ptr() != values.data_ptr()      # the input is correct_ids: never written
        want = f["b%d_out" % c]
        for b, (lo, hi) in enumerate(zip(f["b_off"][:-1], f["b_off"][1:])):
            assert np.array_equal(got[lo:hi].cpu().numpy(), want[lo:hi]), (c, b)
    # drawn here: the rows change, the lengths and the meta prefix do not; the default stays the per-batch decision
    corr = mdata.Corruptions(("mt", "mn", "rn", "rr"), 4, 1.0)
    got = corr(values, offsets, per_sequence=True)
    assert got.shape == values.shape and not torch.equal(got, values)
    for lo in f["b_off"][:-1]:
        assert torch.equal(got[lo:lo + 11], values[lo:lo + 11])
    assert mdata.Corruptions(("mt",), 1, 0.0)(values, offsets) is values
    with pytest.raises(AssertionError):
        corr(values, offsets, choices=f["b3_choices"])


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    path = tmp_path_factory.mktemp("commu")
    src, trg = rag("a_src"), rag("a_trg")
    write_pair(path, "train", src, trg)
    write_pair(path, "val", src[:12], trg[:12])
    return path


def test_dataset_is_merged_filtered_and_resident(data_dir):
    f = fixture()
    seq_len, kept = int(f["a_seq_len"]), f["a_kept"]
    ids, mask = rag("a_ids"), rag("a_mask", "a_ids_off")
    ds = mds.MusicDataset.from_dir(data_dir, "train", seq_len, DEV)
    assert len(ds) == len(kept) and ds.fields["input_ids"].is_cuda and ds.offsets.is_cuda and ds.offsets.dtype == torch.int64
    assert isinstance(ds.lengths, np.ndarray) and ds.lengths.tolist() == f["a_length"][kept].tolist() and ds.max_len <= seq_len
    assert ds.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(f["a_length"][kept])]).tolist()
    assert ds.fields["input_ids"].cpu().tolist() == np.concatenate([ids[i] for i in kept]).tolist()
    assert ds.fields["input_mask"].cpu().tolist() == np.concatenate([mask[i] for i in kept]).tolist()
    full = mds.MusicDataset.from_dir(data_dir, "train", 2096, DEV)       # seq_len >= 2096: nothing is filtered (preprocess.py:116)
    assert len(full) == 40 and full.fields["input_ids"].cpu().tolist() == f["a_ids"].tolist()
    old = mds.MERGE_CHUNK
    try:
        mds.MERGE_CHUNK = 7                                               # several chunks, the last one partial
        chunked = mds.MusicDataset.from_dir(data_dir, "train", seq_len, DEV)
    finally:
        mds.MERGE_CHUNK = old
    assert torch.equal(chunked.fields["input_ids"], ds.fields["input_ids"]) and torch.equal(chunked.offsets, ds.offsets)
    for split in ("valid", "test"):
        val = mds.MusicDataset.from_dir(data_dir, split, 2096, DEV)
        assert len(val) == 12 and val.fields["input_ids"].cpu().tolist() == np.concatenate(ids[:12]).tolist()


def test_load_data_music_batches_equal_the_reference_collate(data_dir):
    f = fixture()
    seq_len = int(f["a_seq_len"])
    batches = rag("a_batches")
    for tag, bucketing in (("bucket", True), ("fixed", False)):
        loader = mdata.load_data_music("train", 7, str(data_dir), use_bucketing=bucketing, seq_len=seq_len, deterministic=True, loop=False)
        got = list(loader)
        assert len(got) == len(batches) - 1 == len(loader)
        for j, item in enumerate(got):
            assert set(item) == {"input_ids", "input_mask", "length"}
            for k, v in item.items():
                assert v.is_cuda and v.dtype == torch.int32 and np.array_equal(v.cpu().numpy(), f["a_col%d_%s_%s" % (j, tag, k)]), (tag, j, k)
        j = len(batches) - 1                                              # repeated and descending indices
        item = loader.batch(torch.from_numpy(batches[j].astype(np.int64)))
        for k, v in item.items():
            assert np.array_equal(v.cpu().numpy(), f["a_col%d_%s_%s" % (j, tag, k)]), (tag, k)
    # shuffled: the rows of torch's own epoch order
    loader = mdata.load_data_music("train", 7, str(data_dir), seq_len=seq_len, loop=None)
    torch.manual_seed(9)
    want = lr.epoch_batches(len(loader.dataset), 7, True)
    torch.manual_seed(9)
    got = list(loader)
    ids = rag("a_ids")
    for idx, item in zip(want, got):
        rows = [ids[f["a_kept"][i]] for i in idx]
        assert item["length"].cpu().tolist() == [len(r) for r in rows] and item["input_ids"].shape[1] == max(len(r) for r in rows)
        assert all(item["input_ids"][b, :len(r)].cpu().tolist() == r.tolist() for b, r in enumerate(rows))
    # corruption and augmentation on: correct_ids is the augmented row, input_ids its corruption, the rest as before
    it = mdata.load_data_music("train", 8, str(data_dir), True, "mt,mn,rn,rr", 2, 1.0, None, True, seq_len, True, True, augment=True)
    item = next(it)
    assert set(item) == {"input_ids", "input_mask", "length", "correct_ids"} and item["input_ids"].shape == item["correct_ids"].shape
    assert not torch.equal(item["input_ids"], item["correct_ids"]) and torch.equal(item["input_ids"][:, 2:11], item["correct_ids"][:, 2:11])
    first = [ids[f["a_kept"][i]] for i in range(8)]
    assert item["length"].cpu().tolist() == [len(r) for r in first]
    cor = item["correct_ids"].cpu().numpy()
    for b, r in enumerate(first):
        if r[1] in (602, 623) and not np.array_equal(cor[b, :len(r)], r):
            k = (int(cor[b, 1]) - int(r[1])) % 12
            assert np.array_equal(cor[b, 2:len(r)], lr.augment_row(r, k - 12 if k > 5 else k, 0)[0][2:]), b
        else:
            assert np.array_equal(cor[b, 2:len(r)], r[2:]), b


def test_launch_count_does_not_depend_on_the_batch_size(data_dir, monkeypatch):
    """a batch of 2 and a batch of 64 cost the same number of library launches.  The kinds present per slot decide how many
    corruption kernels run, so the decisions are pinned to a pattern both sizes hold: two rows, repeated."""
    pattern = np.array([[0, 1, 2, 3], [1, 0, 3, 2]], np.int32)
    monkeypatch.setattr(mdata.Corruptions, "draw_choices", lambda self, B: pattern[np.arange(B) % 2])
    counts = {}
    for B in (2, 64):
        loader = mdata.load_data_music("train", B, str(data_dir), True, "mt,mn,rn,rr", 4, 1.0, None, True, 2096, True, None, augment=True)
        idx = torch.arange(B) % len(loader.dataset)
        loader.batch(idx)                                                 # warm: allocations, lazy loads
        counts[B] = library_launches(lambda: loader.batch(idx))
    assert len(counts[2]) == len(counts[64]) and sorted(counts[2]) == sorted(counts[64])
    names = set(counts[64])
    assert {"gather_offsets_kernel", "gather_rows_kernel", "augment_rows_kernel", "select_rows_kernel", "ragged_to_padded_kernel"} <= names, names
    # two fields gathered, one augmentation, and per slot two kinds -> two corruption kernels and two selects
    assert counts[64].count("gather_rows_kernel") == 2 and counts[64].count("augment_rows_kernel") == 1
    assert counts[64].count("select_rows_kernel") == 8 and counts[64].count("gather_offsets_kernel") == 1


def test_train_loop_consumes_the_loader(data_dir, tmp_path):
    """one TrainLoop step at the tiny model shape of tests/test_host_cpu.py's factory test, fed by next(loader) with corruption
    and augmentation on"""
    from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    from musediffusion_amd.models.network import TransformerNetModel
    from musediffusion_amd.utils.train_util import TrainLoop
    torch.manual_seed(0)
    np.random.seed(0)
    seq_len = 128
    model = TransformerNetModel(32, 32, 32, 729, seq_len, dropout=0.1, bert_hidden=64, bert_layers=2, bert_heads=4, bert_ffn=256,
                                compute_dtype="fp32").train().to(DEV)
    diff = SpacedDiffusion(use_timesteps=space_timesteps(2000, [2000]), betas=get_named_beta_schedule("sqrt", 2000),
                           rescale_timesteps=True, predict_xstart=True)
    data = mdata.load_data_music("train", 4, str(data_dir), True, "mt,mn,rn,rr", 2, 0.5, None, False, seq_len, False, True, augment=True)
    logs = []
    loop = TrainLoop(model=model, diffusion=diff, data=data, batch_size=4, microbatch=4, lr=1e-3, ema_rate="0.9", log_interval=1,
                     save_interval=100, resume_checkpoint="", checkpoint_path=str(tmp_path), learning_steps=1, log_fn=logs.append)
    loop.run_loop()
    assert loop.step == 1 and any("loss" in d and np.isfinite(d["loss"]) for d in logs)
