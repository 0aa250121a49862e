"""GPU: csrc/encode.hip through the C ABI against the reference's recorded answers (tests/golden/encode.npz) and, at batch scale,
against the numpy restatement (tests/encode_ref.py, itself pinned by the fixture in tests/test_encode_cpu.py).  Integer work: every
comparison is exact.  Outputs start filled with a sentinel and carry a guard band behind them that must come back untouched; the
hostile rows (negative and oversized counts, time bases that make no sense, capacities one short) are legal input that must end
in a status - no test here tries to provoke a fault."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import encode_ref as er  # noqa: E402
from musediffusion_amd import _lib, sampling  # noqa: E402
from musediffusion_amd.data.wrapper import collate_batches  # noqa: E402
from musediffusion_amd.utils import decode_util as mdec  # noqa: E402
from musediffusion_amd.utils import encode_util as menc  # noqa: E402
from test_encode_cpu import fixture, fixture_cases, merge_cases, meta_cases  # noqa: E402

DEV = "cuda"
SENTINEL, GUARD = -77, 64
OK, OVERFLOW = er.OK, er.OVERFLOW


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def guarded(shape, dtype=torch.int32):
    """a sentinel-filled buffer of `shape` with GUARD more sentinel elements behind it -> (flat buffer, view of the payload)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, device=DEV, dtype=dtype)
    return buf, buf[:n].view(*shape)


def check_guards(bufs):
    for k, (buf, view) in bufs.items():
        assert bool((buf[view.numel():] == SENTINEL).all()), "guard band behind %s was written" % k


def run_encode(p, ld):
    """mh_encode_events through the C ABI on er.pack()'s arrays, outputs sentinel-filled and guarded -> dict of numpy arrays"""
    B, max_notes, max_slots = len(p["n_notes"]), p["notes"].shape[1], p["slots"].shape[1]
    ins = {k: dev(p[k]) for k in ("notes", "n_notes", "params", "slots", "n_slots")}
    bufs = {k: guarded(s) for k, s in (("words", (B, ld)), ("length", (B,)), ("counts", (B, 2)), ("status", (B,)))}
    v = {k: b[1] for k, b in bufs.items()}
    _lib.check(_lib.lib().mh_encode_events(ins["notes"].data_ptr(), ins["n_notes"].data_ptr(), ins["params"].data_ptr(), ins["slots"].data_ptr(),
                                           ins["n_slots"].data_ptr(), v["words"].data_ptr(), v["length"].data_ptr(), v["counts"].data_ptr(),
                                           v["status"].data_ptr(), B, max_notes, max_slots, ld, _lib.current_stream()), "mh_encode_events")
    torch.cuda.synchronize()
    check_guards(bufs)
    return {k: x.cpu().numpy() for k, x in v.items()}


def run_merge(src, words, lengths, status=None, src_len=None, cap=None):
    """mh_merge_and_mask through the C ABI, outputs sentinel-filled and guarded -> dict of numpy arrays"""
    src, words = np.atleast_2d(src), np.atleast_2d(words)
    B, S, ld = len(words), src.shape[1], words.shape[1]
    cap = B * (S + 1 + 2 * ld) if cap is None else cap
    bufs = {k: guarded(s, t) for k, s, t in (("ids", (cap,), torch.int32), ("mask", (cap,), torch.int32), ("offsets", (B + 1,), torch.int64),
                                             ("length", (B,), torch.int32), ("status", (B,), torch.int32))}
    v = {k: b[1] for k, b in bufs.items()}
    s, w, n = dev(src), dev(words), dev(lengths)
    st = None if status is None else dev(status)
    sl = None if src_len is None else dev(src_len)
    _lib.check(_lib.lib().mh_merge_and_mask(s.data_ptr(), _lib.ptr(sl), w.data_ptr(), n.data_ptr(), _lib.ptr(st), v["ids"].data_ptr(),
                                            v["mask"].data_ptr(), v["offsets"].data_ptr(), v["length"].data_ptr(), v["status"].data_ptr(),
                                            B, S, ld, cap, _lib.current_stream()), "mh_merge_and_mask")
    torch.cuda.synchronize()
    check_guards(bufs)
    return {k: x.cpu().numpy() for k, x in v.items()}


def check_encode(out, rows, ld):
    """kernel outputs == (words, counts, status) rows of the restatement or the fixture"""
    for b, (words, counts, st) in enumerate(rows):
        assert out["status"][b] == st, (b, out["status"][b], st)
        n = len(words) if st == OK else 0
        assert out["length"][b] == n, (b, out["length"][b], n)
        assert np.array_equal(out["words"][b, :n], words[:n]) and not out["words"][b, n:].any(), b
        assert tuple(out["counts"][b]) == (tuple(counts) if st == OK else (0, 0)), (b, out["counts"][b], counts)


def check_merge(out, src_rows, word_rows, statuses):
    """ragged outputs == merge_row of every OK row; the values are packed back to back in row order"""
    at = 0
    for b, (src, words, st) in enumerate(zip(src_rows, word_rows, statuses)):
        ids, mask = er.merge_row(src, words) if st == OK else ([], [])
        assert out["status"][b] == st and out["length"][b] == len(ids), (b, out["status"][b], out["length"][b], len(ids))
        assert out["offsets"][b] == at, b
        assert out["ids"][at:at + len(ids)].tolist() == ids and out["mask"][at:at + len(ids)].tolist() == mask, b
        at += len(ids)
    assert out["offsets"][len(word_rows)] == at
    assert (out["ids"][at:] == SENTINEL).all() and (out["mask"][at:] == SENTINEL).all()


def test_c_abi_reproduces_every_fixture_case():
    """one launch per case (B = 1, buffers of the case's own size) so that every output of every case has its guard band"""
    src = fixture()["src"]
    for c in fixture_cases():
        p = er.pack([dict(notes=c.notes, params=c.params, names=c.names)])
        ld = max(1, len(c.words))                                   # exactly what the row needs
        out = run_encode(p, ld)
        assert out["status"][0] == c.status, (c.name, out["status"][0], c.status)
        if c.status == OK:
            assert out["length"][0] == len(c.words) and np.array_equal(out["words"][0], c.words), c.name
            assert out["counts"][0, 1] == c.oov, c.name
        ref = er.encode_events(c.notes, len(c.notes), c.params, p["slots"][0], int(p["n_slots"][0]), ld)   # and the event count
        check_encode(out, [ref], ld)
        m = run_merge(src, out["words"], out["length"], out["status"])
        n = c.length if c.status == OK else 0                       # a row that did not encode merges to nothing and keeps its status
        assert m["status"][0] == c.status and m["length"][0] == n, c.name
        assert m["offsets"].tolist() == [0, n], c.name
        assert np.array_equal(m["ids"][:n], c.ids[:n]) and np.array_equal(m["mask"][:n], c.mask[:n]), c.name
        assert (m["ids"][n:] == SENTINEL).all() and (m["mask"][n:] == SENTINEL).all(), c.name
    for mc in merge_cases():
        m = run_merge(src, mc.trg, [len(mc.trg)])
        assert m["status"][0] == OK and m["length"][0] == mc.length and m["offsets"].tolist() == [0, mc.length], mc.name
        assert np.array_equal(m["ids"][:mc.length], mc.ids) and np.array_equal(m["mask"][:mc.length], mc.mask), mc.name


BATCH = {}


def batch():
    """64 generated rows of mixed lengths, statuses and time signatures, and the restatement's answers (computed once, never modified)"""
    if not BATCH:
        items, kinds = er.make_batch(2)
        p = er.pack(items)
        BATCH.update(items=items, kinds=kinds, p=p, ld=1024, rows=er.encode_rows(p, 1024))
    return BATCH


def test_batch_composition_is_what_the_batch_test_needs():
    """on the CPU, from the restatement alone"""
    bt = batch()
    st = [r[2] for r in bt["rows"]]
    assert len(st) == 64 and sum(s == OK for s in st) >= 44
    for s in (er.EMPTY, er.NO_CHORDS, er.BAD_TIMEBASE, er.BAD_CHORDS):
        assert st.count(s) >= 4, s
    ok = [b for b in range(64) if st[b] == OK]
    assert len({(int(bt["p"]["params"][b, 1]), int(bt["p"]["params"][b, 2])) for b in ok}) == 4
    assert len({int(bt["p"]["params"][b, 0]) for b in ok}) >= 3 and {int(bt["p"]["params"][b, 4]) for b in ok} == {0, 1}
    assert min(len(bt["rows"][b][0]) for b in ok) < 200 and max(len(bt["rows"][b][0]) for b in ok) > 600
    assert sum(bt["rows"][b][1][1] > 0 for b in ok) >= 8
    assert sum(bt["rows"][b][1][0] < bt["p"]["params"][b, 3] + 4 * bt["p"]["n_notes"][b] + 2 for b in ok) >= 4   # rows that lose notes


def test_kernels_match_the_restatement_at_batch_scale():
    test_batch_composition_is_what_the_batch_test_needs()
    bt = batch()
    out = run_encode(bt["p"], bt["ld"])
    check_encode(out, bt["rows"], bt["ld"])
    g = np.random.default_rng(4)
    src = g.integers(560, 729, (64, 11)).astype(np.int32)
    m = run_merge(src, out["words"], out["length"], out["status"])
    check_merge(m, src, [r[0] for r in bt["rows"]], [r[2] for r in bt["rows"]])
    # without a status the failed rows are empty word rows: src + [1]; a shorter src per row
    src_len = g.integers(0, 12, 64).astype(np.int32)
    m = run_merge(src, out["words"], out["length"], None, src_len)
    check_merge(m, [src[b, :src_len[b]] for b in range(64)], [r[0] for r in bt["rows"]], [OK] * 64)


def test_capacities_one_short_give_overflow_and_write_nothing_past_the_buffer():
    bt = batch()
    ok = [b for b in range(64) if bt["rows"][b][2] == OK]
    need = sorted(len(bt["rows"][b][0]) for b in ok)
    for ld in (need[len(need) // 2] - 1, need[len(need) // 2], need[0] - 1, need[-1]):
        rows = er.encode_rows(bt["p"], ld)
        if ld < need[-1]:
            assert any(r[2] == OVERFLOW for r in rows)
        check_encode(run_encode(bt["p"], ld), rows, ld)
    # the notes / slots buffers one short of a row's count (the count says more than the buffer holds)
    p = dict(bt["p"])
    b = ok[0]
    p["n_notes"] = p["n_notes"].copy()
    p["n_notes"][b] = p["notes"].shape[1] + 1
    rows = er.encode_rows(p, 1024)
    assert rows[b][2] == OVERFLOW
    check_encode(run_encode(p, 1024), rows, 1024)
    # merge: a capacity one short of the total cuts the last non-empty row and leaves the values before it intact
    out = run_encode(bt["p"], 1024)
    src = np.tile(fixture()["src"], (64, 1))
    full = run_merge(src, out["words"], out["length"], out["status"])
    total = int(full["offsets"][-1])
    last = max(b for b in range(64) if full["length"][b] > 0)
    cut = run_merge(src, out["words"], out["length"], out["status"], cap=total - 1)
    assert cut["status"][last] == OVERFLOW and cut["length"][last] == 0 and cut["offsets"][-1] == full["offsets"][last]
    assert np.array_equal(cut["length"][:last], full["length"][:last]) and np.array_equal(cut["offsets"][:last + 1], full["offsets"][:last + 1])
    n = int(full["offsets"][last])
    assert np.array_equal(cut["ids"][:n], full["ids"][:n]) and (cut["ids"][n:] == SENTINEL).all() and (cut["mask"][n:] == SENTINEL).all()
    tiny = run_merge(src, out["words"], out["length"], out["status"], cap=5)
    assert (tiny["ids"] == SENTINEL).all() and not tiny["length"].any() and not tiny["offsets"].any()
    assert all(tiny["status"][b] == (OVERFLOW if full["length"][b] else full["status"][b]) for b in range(64))


def test_hostile_counts_and_parameters_end_in_a_status():
    bt = batch()
    p = {k: v.copy() for k, v in bt["p"].items()}
    ok = [b for b in range(64) if bt["rows"][b][2] == OK]
    p["n_notes"][ok[0]] = -5
    p["n_notes"][ok[1]] = 2 ** 31 - 1
    p["n_slots"][ok[2]] = p["slots"].shape[1] + 1
    p["n_slots"][ok[3]] = -1
    p["n_slots"][ok[4]] = 2 ** 31 - 1
    p["params"][ok[5]] = (2 ** 31 - 1, 2 ** 31 - 1, 1, 4, 0)
    p["params"][ok[6]] = (480, 4, 0, 4, 0)
    p["params"][ok[7], 3] = 2 ** 31 - 1                              # measures: more units than the kernel sorts
    p["params"][ok[8], 3] = -7
    p["params"][ok[9], 4] = 5                                        # any non-zero is "incomplete"
    p["params"][ok[10]] = (1, 4, 4, 4, 0)
    p["notes"][ok[11]] = np.random.default_rng(0).integers(-2 ** 31, 2 ** 31 - 1, p["notes"][ok[11]].shape)
    p["notes"][ok[12], :, 1] = 2 ** 31 - 1
    p["notes"][ok[13], :, 0] = 2 ** 31 - 1
    p["slots"][ok[14]] = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31 - 1, p["slots"][ok[14]].shape)
    rows = er.encode_rows(p, 1024)
    assert [rows[ok[k]][2] for k in range(11)] == [er.EMPTY, OVERFLOW, OVERFLOW, er.NO_CHORDS, OVERFLOW, er.BAD_TIMEBASE, er.BAD_TIMEBASE,
                                                   OVERFLOW, OK, OK, er.BAD_TIMEBASE]
    out = run_encode(p, 1024)
    check_encode(out, rows, 1024)
    lengths = out["length"].copy()
    lengths[ok[0]], lengths[ok[1]], lengths[ok[2]] = -3, 2 ** 31 - 1, 1025   # lengths that lie: clamped to [0, ld]
    m = run_merge(np.tile(fixture()["src"], (64, 1)), out["words"], lengths)
    words = [out["words"][b, :min(max(int(lengths[b]), 0), 1024)] for b in range(64)]
    check_merge(m, [fixture()["src"]] * 64, words, [OK] * 64)


def clean_cases():
    return [c for c in fixture_cases() if c.clean and c.status == OK and int(c.params[0]) == 480]


def test_round_trip_through_the_python_surface():
    """encode_notes -> merge_and_mask -> collate_batches -> split_meta_midi returns the words; decoding that and encoding the decoded
    notes again returns the same words (the flagged-clean fixture cases at 480 ticks per beat, the decoder's tick base)"""
    cs = clean_cases()
    assert len(cs) >= 20
    src = fixture()["src"]
    enc = menc.encode_notes(*menc.pack_items([c.notes for c in cs], [c.params for c in cs], [c.names for c in cs]))
    assert isinstance(enc, menc.EncodedBatch) and enc.words.is_cuda and mdec.encode_notes is menc.encode_notes
    rows = enc.cpu()
    for c, w, st, cnt in zip(cs, rows.words, rows.status, rows.counts):
        assert st == OK and np.array_equal(w, c.words) and cnt[1] == c.oov, c.name
    fields, offsets, length, status = menc.merge_and_mask(np.tile(src, (len(cs), 1)), enc.words, enc.lengths, enc.status)
    assert offsets.dtype == torch.int64 and length.cpu().tolist() == [c.length for c in cs] and not status.cpu().any()
    L = max(c.length for c in cs) + 5
    cond = collate_batches(fields, offsets, L)
    for b, c in enumerate(cs):
        assert cond["input_ids"][b, :c.length].cpu().tolist() == c.ids.tolist() and cond["input_mask"][b, :c.length].cpu().tolist() == c.mask.tolist()
    restored, lengths, meta, st = mdec.split_meta_midi(cond["input_ids"], cond["input_mask"])
    restored, lengths = restored.cpu().numpy(), lengths.cpu().numpy()
    assert not st.cpu().any() and np.array_equal(meta.cpu().numpy(), np.tile(src, (len(cs), 1)))
    for b, c in enumerate(cs):
        assert np.array_equal(restored[b, :lengths[b]], c.words), c.name
    # decode -> encode again returns the same words.  This holds where the words hold every note with all four of its words inside a
    # measure that has its Bar (the decoder counts Bars to place a note; a note whose Note On was unknown is no note to it), so those
    # cases are chosen from the fixture's INPUTS: no OOV line, every input note encoded, every note before measure num_measures.
    # The decoded notes sit on the position / duration / velocity grids, where encoding is the identity.
    ts_token = {(4, 4): 627, (3, 4): 628, (6, 8): 629, (12, 8): 630}
    ids = cond["input_ids"].clone()
    for b, c in enumerate(cs):
        ids[b, 2] = ts_token[(int(c.params[1]), int(c.params[2]))]    # the fixture's meta says 4/4 for every case
    dec = mdec.decode_tokens(ids, cond["input_mask"]).cpu()
    again = []
    for b, c in enumerate(cs):
        bars, chords = int((c.words == 2).sum()), int(((c.words >= 195) & (c.words <= 303)).sum())
        T = er.timebase(*c.params[:3])[0]
        if c.oov == 0 and 4 * len(c.notes) == len(c.words) - 1 - bars - 2 * chords and c.notes[:, 0].max() < int(c.params[3]) * T:
            assert dec.status[b] == mdec.OK and len(dec.notes[b]) == len(c.notes), c.name
            again.append((dec.notes[b], c))
    assert len(again) >= 12 and {(int(c.params[1]), int(c.params[2])) for _, c in again} >= {(4, 4), (3, 4), (6, 8)}
    enc2 = menc.encode_notes(*menc.pack_items([a[0] for a in again], [a[1].params for a in again], [a[1].names for a in again])).cpu()
    for (notes, c), w, st2 in zip(again, enc2.words, enc2.status):
        assert st2 == OK and np.array_equal(w, c.words), c.name


def test_meta_to_batch_dict_and_tokens_on_the_device():
    name, meta, tokens, _ = meta_cases()[0]
    a, b = mdec.meta_to_batch(tokens, 3, 48), mdec.meta_to_batch(dict(meta), 3, 48)
    for k in ("input_ids", "input_mask"):
        assert torch.equal(a[k], b[k]) and a[k].is_cuda and a[k].dtype == torch.int32
    ids, mask = a["input_ids"].cpu().numpy(), a["input_mask"].cpu().numpy()
    n = len(tokens)
    assert (ids[:, :n] == np.array(tokens)).all() and not ids[:, n:].any() and not mask[:, :n + 1].any() and mask[:, n + 1:].all()


def test_encode_batch_feeds_sampling_modify(tmp_path):
    """(MIDI file or note array, meta dict) pairs -> cond -> sampling.modify on a tiny model: rows come back with the encoded meta as prefix"""
    from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    from musediffusion_amd.models.network import TransformerNetModel
    from oracle import denoiser as odn
    E, H, F, nL, nh, V, L, Tt = 32, 64, 256, 2, 4, 729, 96, 32
    model = TransformerNetModel(E, E, Tt, V, L, dropout=0.0, bert_hidden=H, bert_layers=nL, bert_heads=nh, bert_ffn=F, compute_dtype="fp32")
    model.load_state_dict(odn.random_state_dict(E, H, F, nL, V, L, Tt, seed=21, emb_std=1.0))
    model.eval().requires_grad_(False).to(DEV)
    diff = SpacedDiffusion(use_timesteps=space_timesteps(2000, [2000]), betas=get_named_beta_schedule("sqrt", 2000),
                           rescale_timesteps=True, predict_xstart=True)
    diff.noise_fn, diff.rng_mode = None, "philox"
    name, meta, tokens, _ = meta_cases()[0]
    meta = dict(meta, num_measures=4, chord_progression="-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 4 + ["E"] * 4 + ["Am"] * 8))
    T = 1920
    notes = np.array([[0, 240, 57, 80], [480, 960, 60, 90], [T, T + 480, 55, 70], [2 * T + 960, 3 * T, 53, 100], [3 * T, 3 * T + 240, 57, 64]], np.int32)
    path = str(tmp_path / "in.mid")
    mdec.write_midi(path, notes, [], [584, 623, 627])
    many = np.concatenate([notes + np.array([k * 7, k * 7, 0, 0], np.int32) for k in range(12)])     # too long for seq_len 96
    items = [(notes, meta), (path, meta), (many, meta), (notes[:0], meta), (notes, dict(meta, audio_key="cmajor", is_incomplete_measure=True))]
    cond, report = menc.encode_batch(items, L)
    assert report["kept"].tolist() == [0, 1, 4] and report["status"].tolist() == [OK, OK, OK, er.EMPTY, OK] and report["length"][2] > L
    assert set(cond) == {"input_ids", "input_mask", "length"} and cond["input_ids"].shape == (3, L) and cond["input_ids"].is_cuda
    ids = cond["input_ids"].cpu().numpy()
    assert np.array_equal(ids[0], ids[1])                             # the file holds what the array holds
    want = er.merge_row(menc.MetaToSequence().encode_meta(meta), er.encode_events(notes, 5, (480, 4, 4, 4, 0), er.chord_slots(meta["chord_progression"].split("-")), 32, 4096)[0])
    n = len(want[0])
    assert ids[0, :n].tolist() == want[0] and not ids[0, n:].any() and cond["length"].cpu().tolist()[0] == n
    assert cond["input_mask"][0].cpu().tolist() == want[1] + [1] * (L - n)
    tok = sampling.modify(model, diff, cond, step=20, strength=0.5, sharded=False)
    assert tok.shape == (3, L) and tok.is_cuda
    tok = tok.cpu().numpy()
    for b in range(3):
        k = int((cond["input_mask"][b] == 0).sum())                   # meta + chord pairs + EOS: anchored
        assert np.array_equal(tok[b, :k], ids[b, :k]) and tok[b, :11].tolist() == menc.MetaToSequence().encode_meta(items[report["kept"][b]][1])
