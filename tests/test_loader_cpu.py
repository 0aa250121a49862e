"""CPU: the dataset loader's restatement (tests/loader_ref.py) against every record of tests/golden/loader.npz - what the reference's own
helper_tokenize / helper_filter / collate_batches, Corruptions.__call__, augment.py and Preprocessor answered
(tools/make_golden_loader.py) - bit for bit; the epoch order against torch.utils.data.DataLoader; the host side of
musediffusion_amd.data.dataset (file names, the missing-file error, the `loop` forms).  No kernel runs here: the device side is
tests/test_loader_gpu.py."""
import itertools
import random

import numpy as np
import pytest
import torch

from conftest import load_golden

import encode_ref as er
import loader_ref as lr
from musediffusion_amd import data as mdata
from musediffusion_amd.data import corruption as mcorr
from musediffusion_amd.data import dataset as mds
from musediffusion_amd.utils import encode_util as menc
from oracle import batch as ob

FIX = {}


def fixture():
    if not FIX:
        FIX.update(load_golden("loader.npz"))
    return FIX


def rag(name, off=None):
    f = fixture()
    return lr.rows_of(f[name], f[off or name + "_off"])


# ------------------------------------------------------------------------------------------------------------------ (a)
def test_merge_filter_and_collate_records():
    f = fixture()
    src, trg, ids, mask = rag("a_src"), rag("a_trg"), rag("a_ids"), rag("a_mask", "a_ids_off")
    assert len(src) == 40
    for b in range(40):
        got_ids, got_mask = er.merge_row(src[b], trg[b])
        assert got_ids == ids[b].tolist() and got_mask == mask[b].tolist() and f["a_length"][b] == len(got_ids), b
    seq_len = int(f["a_seq_len"])
    kept = np.nonzero(f["a_length"] <= seq_len)[0]                        # helper_filter: length <= seq_len
    assert np.array_equal(kept, f["a_kept"]) and 0 < len(kept) < 40 and seq_len < mds.FILTER_BELOW
    batches = rag("a_batches")
    assert len(batches) >= 5
    for j, idx in enumerate(batches):
        rows, masks = [ids[kept[i]] for i in idx], [mask[kept[i]] for i in idx]
        for tag, L in (("bucket", None), ("fixed", seq_len)):
            want = ob.collate(rows, masks, rows, L)
            for k in ("input_ids", "input_mask", "length"):
                assert np.array_equal(want[k], f["a_col%d_%s_%s" % (j, tag, k)]), (j, tag, k)
            assert "a_col%d_%s_correct_ids" % (j, tag) not in f


# ------------------------------------------------------------------------------------------------------------------ (b)
def corruption_draws(c):
    f = fixture()
    return dict(u=f["b%d_u" % c], new=f["b%d_new" % c], pairs=f["b%d_pairs" % c])


def test_per_sequence_corruption_records():
    f = fixture()
    available = [str(a) for a in f["b_available"]]
    assert available == ["mt", "mn", "rn", "rr"] and f["b_configs"].tolist() == [[2, 0.5], [4, 0.5], [2, 1.0], [4, 1.0]]
    for c, (corr_max, corr_p) in enumerate(f["b_configs"]):
        ch = f["b%d_choices" % c]
        assert ch.shape == (16, int(corr_max)) and ch.max() == 3
        if corr_p == 1.0:                                                # every slot fires, and a row never takes one kind twice
            assert (ch >= 0).all() and all(len(set(r)) == len(r) for r in ch.tolist())
        got = lr.corrupt_per_sequence(f["b_values"], f["b_off"], ch, available, corruption_draws(c))
        assert np.array_equal(got, f["b%d_out" % c]), c
    assert not np.array_equal(f["b3_out"], f["b_values"])
    rows, masks, cor = rag("b_values", "b_off"), rag("b_mask", "b_off"), lr.rows_of(f["b0_out"], f["b_off"])
    for tag, L in (("bucket", None), ("fixed", max(len(r) for r in rows) + 3)):
        want = ob.collate(cor, masks, rows, L)
        for k in ("input_ids", "input_mask", "length", "correct_ids"):
            assert np.array_equal(want[k], f["b_col_%s_%s" % (tag, k)]), (tag, k)


def test_draw_choices_makes_the_reference_decision_per_row():
    """shuffle, then one random() per kept slot (corruption.py:51-55), restated here on Python's own generator"""
    corr = mdata.Corruptions(("mt", "mn", "rn", "rr"), 3, 0.5)
    mcorr.generator.seed(77)
    got = corr.draw_choices(9)
    g = random.Random(77)
    want = np.full((9, 3), -1, np.int32)
    for b in range(9):
        order = [0, 1, 2, 3]
        g.shuffle(order)
        for r in range(3):
            if g.random() > 0.5:
                want[b, r] = order[r]
    assert got.dtype == np.int32 and np.array_equal(got, want) and (got >= 0).any() and (got < 0).any()
    assert (mdata.Corruptions(("mt", "rr"), 2, 0.0).draw_choices(5) == -1).all()


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_augmentation_tables():
    """Key numbers and chord names as augment_by_key and sync_key_augment give them, for every key_change and both origins; tempo
    tokens as encode_bpm gives them.  The tempo token map works on the token, so it equals encode_bpm(bpm + 5 c) wherever the token
    still determines the tempo bin: bpm <= 204 (above, min(bpm, 200) saturates at 600 and the reference, which knows the tempo itself,
    can stay at 600 where the token map steps down) and bpm + 5 c >= 0 (a negative tempo gives the reference a negative bin, which no
    token stands for; the clamp at bin 1 is the project's).  Outside that range the record is checked against the reference's own
    formula, so that every entry of the table is pinned."""
    f = fixture()
    for o, origin in enumerate((602, 623)):
        for k in lr.KEY_CHANGES:
            assert lr.key_token(origin, k) == 602 + f["c_key_numbers"][o, k + 6], (origin, k)
    assert f["c_key_numbers"][0].tolist() == [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]
    names = [str(n) for n in f["c_chord_names"]]
    assert len(names) == 108 + 45
    vocab = menc.CHORD_VOCABULARY
    assert vocab == er.CHORD_VOCABULARY
    for o in range(2):
        for k in lr.KEY_CHANGES:
            for name, synced in zip(names, f["c_chord_synced"][o, k + 6]):
                assert lr.chord_token(vocab[name.lower()], k) == vocab[str(synced).lower()], (o, k, name, synced)
                assert lr.rotate_name(name, k) == str(synced), (k, name, synced)
    assert lr.chord_token(303, 5) == 303 and lr.chord_token(194, 1) == 194 and lr.chord_token(304, 1) == 304
    bpm, tok = f["c_bpm"], f["c_bpm_tokens"]
    assert bpm.tolist() == list(range(5, 221)) and tok.shape == (216, 5)
    enc = lambda b: 560 + (min(b, 200) // 5 or 1)                         # encode_bpm + its offset
    checked = 0
    for i, b in enumerate(bpm.tolist()):
        for c in lr.BPM_CHANGES:
            assert tok[i, c + 2] == enc(b + 5 * c), (b, c)
            if b <= 204 and b + 5 * c >= 0:
                assert lr.tempo_token(enc(b), c) == tok[i, c + 2], (b, c)
                checked += 1
    assert checked == 5 * 200 - 5 and lr.tempo_token(560, 2) == 560 and lr.tempo_token(561, -2) == 561 and lr.tempo_token(600, 2) == 600


# ------------------------------------------------------------------------------------------------------------------ (d)
def d_rows():
    """-> list of (case index, k, c, status, ids, mask) and the per-case inputs"""
    f = fixture()
    ids, mask = rag("d_ids"), rag("d_mask", "d_ids_off")
    return [(int(f["d_case"][i]), int(f["d_key_change"][i]), int(f["d_bpm_change"][i]), int(f["d_status"][i]), ids[i], mask[i])
            for i in range(len(ids))]


def d_cases():
    f = fixture()
    fields = [str(x) for x in f["d_meta_fields"]]
    out = []
    for i, name in enumerate(f["d_name"]):
        meta = dict(zip(fields, (str(v) for v in f["d_meta_values"][i])))
        for k in ("bpm", "min_velocity", "max_velocity"):
            meta[k] = int(meta[k])
        meta["num_measures"] = float(meta["num_measures"])
        meta["inst"] = meta["inst"].split("-")[0]                         # MetaParser.remove_number_from_inst
        out.append(dict(name=str(name), notes=f["d_notes"][f["d_notes_off"][i]:f["d_notes_off"][i + 1]],
                        names=[str(n) for n in f["d_chords"][f["d_chords_off"][i]:f["d_chords_off"][i + 1]]], meta=meta))
    return out


def project_row(case, k=0):
    """the project's own encoding of a case (restatement: MetaToSequence + tests/encode_ref.py), notes and names moved by k"""
    notes = case["notes"].copy()
    notes[:, 2] += k
    names = [lr.rotate_name(n, k) for n in case["names"]]
    params = (480, 4, 4, int(np.ceil(case["meta"]["num_measures"])), 0)
    words, _, st = er.encode_events(notes, len(notes), params, er.chord_slots(names), len(names), 4096)
    assert st == er.OK
    return er.merge_row(menc.MetaToSequence().encode_meta(case["meta"]), words)


def test_token_map_equals_the_file_level_augmentation():
    """every recorded variant == augment_row(the case's unaugmented row); the files the reference dropped are PITCH_RANGE, the case
    whose key is no origin is NOT_ORIGIN; no chord name had to be left out"""
    f = fixture()
    assert f["d_root_twice"].tolist() == [""]
    cases, rows = d_cases(), d_rows()
    assert len(cases) == 20 and len(rows) == 200
    base = {ci: ids for ci, k, c, st, ids, _ in rows if (k, c) == (0, 0) and st == 0}
    seen = {0: 0, 1: 0, 2: 0}
    for ci, k, c, st, ids, mask in rows:
        seen[st] += 1
        if ci in base:
            got, status = lr.augment_row(base[ci], k, c)
            assert status == (lr.AUGMENT_OK, None, lr.PITCH_RANGE)[st], (cases[ci]["name"], k, c, status)
            if st == 0:
                assert np.array_equal(got, ids), (cases[ci]["name"], k, c)
                assert np.array_equal(mask, (np.arange(len(ids)) > np.nonzero(ids == 1)[0][0]).astype(np.int32))
            else:
                assert np.array_equal(got, base[ci])
        else:                                                             # no variant at all: the project's own encoding is the row
            assert st == 1 and cases[ci]["meta"]["audio_key"] == "dmajor"
            row = np.array(project_row(cases[ci])[0], np.int32)
            got, status = lr.augment_row(row, k, c)
            assert status == lr.NOT_ORIGIN and np.array_equal(got, row)
    assert seen[0] >= 150 and seen[1] == 10 and seen[2] >= 4
    assert {k for _, k, c, st, _, _ in rows if st == 0} == {-6, -5, -3, -1, 0, 1, 2, 3, 4, 5} and {c for _, k, c, _, _, _ in rows} == {-2, -1, 0, 1, 2}
    # the unaugmented rows are what the project's own encoder makes of the notes, and so is every variant of the moved notes
    for ci, k, c, st, ids, mask in rows:
        if st == 0 and c == 0:
            want_ids, want_mask = project_row(cases[ci], k)
            want_ids[1] = lr.key_token(want_ids[1], k)
            assert want_ids == ids.tolist() and want_mask == mask.tolist(), (cases[ci]["name"], k)


def test_augment_row_statuses_and_hostile_rows():
    row = np.array([580, 602, 627, 633, 639, 644, 651, 660, 700, 720, 727, 432, 195, 1, 2, 432, 150, 60, 320, 440, 303, 1], np.int32)
    got, st = lr.augment_row(row, 3, -1)
    assert st == lr.AUGMENT_OK and got.tolist() == [579, 605, 627, 633, 639, 644, 651, 660, 700, 720, 727, 432, 222, 1, 2, 432, 150, 63, 320, 440, 303, 1]
    assert lr.augment_row(row[:11], 0, 0)[1] == lr.BAD_ROW and lr.augment_row(row, 6, 0)[1] == lr.BAD_ROW and lr.augment_row(row, 0, 3)[1] == lr.BAD_ROW
    hi = row.copy()
    hi[17] = 3 + 127 - 5 + 1                                              # one out of range for k = 5
    assert lr.augment_row(hi, 5, 0)[1] == lr.PITCH_RANGE and lr.augment_row(hi, 4, 0)[1] == lr.AUGMENT_OK
    hostile = row.copy()
    hostile[2:11] = [60, 200, 3, 130, 195, 302, 303, 64, 250]             # pitch- and chord-valued tokens inside the first 11: copied
    got, st = lr.augment_row(hostile, -6, 2)
    assert st == lr.AUGMENT_OK and got[2:11].tolist() == hostile[2:11].tolist() and got[17] == 54
    other = row.copy()
    other[1] = 603
    assert lr.augment_row(other, 1, 1)[1] == lr.NOT_ORIGIN
    assert mds.KEY_CHANGES == lr.KEY_CHANGES and mds.BPM_CHANGES == lr.BPM_CHANGES
    assert (mds.AUGMENT_OK, mds.NOT_ORIGIN, mds.PITCH_RANGE, mds.BAD_ROW) == (lr.AUGMENT_OK, lr.NOT_ORIGIN, lr.PITCH_RANGE, lr.BAD_ROW)


def test_gather_restatement_edges():
    off = np.array([0, 3, 3, 4, 10], np.int64)
    o, n, s = lr.gather_offsets(off, [3, -1, 0, 4, 1, 2], 100)
    assert o.tolist() == [0, 6, 6, 9, 9, 9, 10] and n.tolist() == [6, 0, 3, 0, 0, 1] and s.tolist() == [0, 1, 0, 1, 0, 0]
    o, n, s = lr.gather_offsets(off, [0, 3, 1, 2], 8)                     # the second row would end at 9 > 8: cut, and so is all after it
    assert o.tolist() == [0, 3, 3, 3, 3] and n.tolist() == [3, 0, 0, 0] and s.tolist() == [0, 2, 0, 2]


# ------------------------------------------------------------------------------------------------------------------ epoch order
def stub_dataset(n):
    lengths = np.arange(12, 12 + n)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]))
    vals = torch.zeros(int(off[-1]), dtype=torch.int32)
    return mds.MusicDataset({"input_ids": vals, "input_mask": vals}, off, lengths, 128)


@pytest.mark.parametrize("batch_size", [1, 7, 64])
@pytest.mark.parametrize("shuffle", [False, True])
def test_epoch_order_is_the_dataloaders(batch_size, shuffle):
    n = 40
    ref = torch.utils.data.DataLoader(list(range(n)), batch_size=batch_size, shuffle=shuffle)
    torch.manual_seed(1234)
    want = [[b.tolist() for b in ref] for _ in range(2)]
    tail = torch.rand(3)
    loader = mds.MusicLoader(stub_dataset(n), batch_size, shuffle)
    torch.manual_seed(1234)
    got = [[b.tolist() for b in loader.index_batches()] for _ in range(2)]
    assert got == want and torch.equal(torch.rand(3), tail)              # the same draws from the default generator, no more, no fewer
    torch.manual_seed(1234)
    assert [lr.epoch_batches(n, batch_size, shuffle) for _ in range(2)] == want
    assert len(loader) == len(ref) == len(want[0]) and len(want[0][-1]) == (n % batch_size or batch_size)   # the last partial batch is kept
    if shuffle:
        assert want[0] != want[1] and sorted(itertools.chain(*want[0])) == list(range(n))


# ------------------------------------------------------------------------------------------------------------------ files, loop forms
def write_pair(path, tag, src, trg):
    for kind, rows in (("input", src), ("target", trg)):
        arr = np.empty(len(rows), dtype=object)
        for i, r in enumerate(rows):
            arr[i] = np.asarray(r, np.int16 if kind == "target" else object)
        np.save(str(path / ("%s_%s.npy" % (kind, tag))), arr, allow_pickle=True)


def test_from_dir_file_names_and_missing_file(tmp_path):
    src, trg = rag("a_src"), rag("a_trg")
    write_pair(tmp_path, "train", src[:30], trg[:30])
    with pytest.raises(FileNotFoundError) as e:
        mds._load_pair(tmp_path, "valid")
    assert "input_val.npy" in str(e.value) and str(tmp_path) in str(e.value)
    write_pair(tmp_path, "val", src[30:], trg[30:])
    s, t = mds._load_pair(tmp_path, "train")
    assert len(s) == len(t) == 30 and [int(x) for x in t[3]] == trg[3].tolist() and [int(x) for x in s[3]] == src[3].tolist()
    for split in ("valid", "test", "VALID"):                              # load_raw_data: 'valid' and 'test' read the val pair
        s, t = mds._load_pair(tmp_path, split)
        assert len(s) == 10 and [int(x) for x in t[0]] == trg[30].tolist()
    with pytest.raises(AssertionError):
        mds._load_pair(tmp_path, "dev")
    (tmp_path / "target_val.npy").unlink()
    for call in (lambda: mds.MusicDataset.from_dir(tmp_path, "test", 128, "cpu"), lambda: mdata.load_data_music("valid", 4, str(tmp_path), seq_len=128),
                 lambda: mdata.load_data_music(["train", "valid"], 4, str(tmp_path / "nowhere"), seq_len=128)):
        with pytest.raises(FileNotFoundError) as e:
            call()
        assert e.value.args[0].count(".npy") >= 1
    with pytest.raises(FileNotFoundError):
        mdata.load_data_music("train", 4, None, seq_len=128)


def test_loop_forms(monkeypatch):
    """loop=True: an infinite iterator; False: one pass per iter(); None: the loader; a list of splits: a list.  The device work is
    replaced by stand-ins here (from_dir -> a host-only dataset, batch -> its indices); tests/test_loader_gpu.py runs the real thing."""
    made = []
    monkeypatch.setattr(mds.MusicDataset, "from_dir", classmethod(lambda cls, d, split, seq_len, device: made.append(split) or stub_dataset(10)))
    monkeypatch.setattr(mds.MusicLoader, "batch", lambda self, idx: idx.tolist())
    kw = dict(batch_size=4, data_dir="x", seq_len=128, deterministic=True, num_preprocess_proc=8, num_loader_proc=3)
    it = mdata.load_data_music("train", loop=True, **kw)
    assert not isinstance(it, mds.MusicLoader) and iter(it) is it
    assert [next(it) for _ in range(7)] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]] * 2 + [[0, 1, 2, 3]]
    once = mdata.load_data_music("valid", loop=False, **kw)
    assert list(once) == list(once) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]] and len(once) == 3
    raw = mdata.load_data_music("test", loop=None, **kw)
    assert isinstance(raw, mds.MusicLoader) and isinstance(once, mds.MusicLoader) and raw.corruption is None and raw.augment is None
    assert not raw.shuffle and raw.use_bucketing and mdata.load_data_music("train", loop=None, **dict(kw, deterministic=False)).shuffle
    both = mdata.load_data_music(("train", "valid"), loop=None, **kw)
    assert isinstance(both, list) and len(both) == 2 and made[-2:] == ["train", "valid"]
    full = mdata.load_data_music("train", loop=None, use_corruption=True, corr_available="mt,mn,rn,rr", corr_max=2, corr_p=0.5,
                                 corr_kwargs="dict(p=0.4)", use_bucketing=False, augment=True, **kw)
    assert isinstance(full.corruption, mdata.Corruptions) and full.corruption.corr_max == 2 and full.corruption.corr_kwargs == {"p": 0.4}
    assert isinstance(full.augment, mdata.Augment) and not full.use_bucketing and full.seq_len == 128
