"""GPU: csrc/decode.hip through the C ABI against the reference's recorded answers (tests/golden/decode.npz) and, at batch
scale, against the numpy restatement (tests/decode_ref.py, itself pinned by the fixture in tests/test_decode_cpu.py).
Integer work: every comparison is exact.  Outputs start filled with a sentinel and carry a guard band behind them that must
come back untouched; the hostile rows (garbage tokens, masks that split anywhere, empty or malformed chord parts) are legal
input that must end in a status - no test here tries to provoke a fault."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
from musediffusion_amd import _lib, metric, sampling  # noqa: E402
from musediffusion_amd.utils import decode_util as mdec  # noqa: E402
from musediffusion_amd.utils.decode_util import OK, OVERFLOW  # noqa: E402
from test_decode_cpu import check_midi_file, fixture_cases  # noqa: E402

DEV = "cuda"
SENTINEL, GUARD = -77, 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def guarded(*shape):
    """a sentinel-filled int32 buffer of `shape` with GUARD more sentinel words behind it -> (flat buffer, view of the payload)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, device=DEV, dtype=torch.int32)
    return buf, buf[:n].view(*shape)


def run_kernels(tokens, masks, ld_out, max_notes, max_chords, strict):
    """both kernels (and mh_validate_tokens between them when strict) through the C ABI on sentinel-filled, guarded outputs"""
    lib, stream = _lib.lib(), _lib.current_stream()
    B, L = tokens.shape
    t, m = dev(tokens), dev(masks)
    bufs = {k: guarded(*shape) for k, shape in (("restored", (B, ld_out)), ("len", (B,)), ("meta", (B, 11)), ("status", (B,)),
                                                ("notes", (B, max_notes, 4)), ("chords", (B, max_chords, 2)), ("counts", (B, 3)))}
    v = {k: b[1] for k, b in bufs.items()}
    _lib.check(lib.mh_restore_chord(t.data_ptr(), m.data_ptr(), v["restored"].data_ptr(), v["len"].data_ptr(), v["meta"].data_ptr(),
                                    v["status"].data_ptr(), B, L, ld_out, stream), "mh_restore_chord")
    split = {k: v[k].cpu().numpy().copy() for k in ("restored", "len", "meta", "status")}
    val = mdec.validate_tokens(v["restored"], v["len"]) if strict else None
    _lib.check(lib.mh_decode_events(v["restored"].data_ptr(), v["len"].data_ptr(), v["meta"].data_ptr(), _lib.ptr(val), int(strict),
                                    v["notes"].data_ptr(), v["chords"].data_ptr(), v["counts"].data_ptr(), v["status"].data_ptr(), B, ld_out,
                                    max_notes, max_chords, stream), "mh_decode_events")
    torch.cuda.synchronize()
    out = {k: x.cpu().numpy() for k, x in v.items()}
    for k, (buf, view) in bufs.items():
        assert bool((buf[view.numel():] == SENTINEL).all()), "guard band behind %s was written" % k
    assert np.array_equal(out["restored"], split["restored"]) and np.array_equal(out["len"], split["len"]), "the event pass wrote its inputs"
    return split, out


def check_against_rows(split, out, rows_split, rows, ld_out):
    """kernel outputs == the restatement's (or the fixture's) rows: rows_split = (restored, meta, status) of split_meta_midi alone"""
    for b, ((restored, meta, st0), r) in enumerate(zip(rows_split, rows)):
        assert split["status"][b] == st0, b
        n = len(restored) if st0 == OK else 0
        assert split["len"][b] == n and np.array_equal(split["restored"][b, :n], restored[:n]) and not split["restored"][b, n:].any(), b
        assert np.array_equal(split["meta"][b], meta), b
        assert out["status"][b] == r["status"], (b, out["status"][b], r["status"])
        assert tuple(out["counts"][b]) == tuple(r["counts"]), b
        k, c = (r["counts"][0], r["counts"][1]) if r["status"] == OK else (0, 0)
        if r["status"] == OK:
            assert np.array_equal(out["notes"][b, :k], r["notes"]) and np.array_equal(out["chords"][b, :c], r["chords"]), b
        if r["status"] != OVERFLOW:                                                  # an overflowing row fills what capacity it has
            assert (out["notes"][b, k:] == SENTINEL).all() and (out["chords"][b, c:] == SENTINEL).all(), b


@pytest.mark.parametrize("strict", [False, True], ids=["once", "strict"])
def test_kernels_reproduce_every_fixture_case(strict):
    """one launch per case (B = 1, the case's own L) so that every output of every case has its guard band"""
    for c in fixture_cases():
        L = len(c.tokens)
        ld_out, max_notes, max_chords = min(2 * L, dr.MAX_ROW), max(1, len(c.notes)), max(1, len(c.marker_time))
        split, out = run_kernels(c.tokens[None], c.mask[None], ld_out, max_notes, max_chords, strict)
        assert split["status"][0] == c.split_status, c.name
        if c.split_ok:
            n = len(c.restored)
            assert split["len"][0] == n and np.array_equal(split["restored"][0, :n], c.restored) and not split["restored"][0, n:].any(), c.name
            assert np.array_equal(split["meta"][0], c.meta), c.name
        else:
            assert split["len"][0] == 0 and not split["restored"][0].any(), c.name
        assert out["status"][0] == c.status[strict], (c.name, out["status"][0], c.status[strict])
        if c.status[strict] == OK:
            assert tuple(out["counts"][0]) == (len(c.notes), len(c.marker_time), c.oov), c.name
            assert np.array_equal(out["notes"][0, :len(c.notes)], c.notes) and np.array_equal(out["chords"][0, :len(c.marker_time), 0], c.marker_time), c.name
            assert [mdec.CHORD_NAMES[t - 195] for t in out["chords"][0, :len(c.marker_time), 1]] == c.marker_text, c.name
        ref = dr.decode_row(c.tokens, c.mask, ld_out, max_notes, max_chords, strict)    # and the parts the fixture does not hold
        check_against_rows(split, out, [dr.split_and_restore(c.tokens, c.mask, ld_out)[:3]], [ref], ld_out)


BATCH = {}


def batch():
    """B = 96, L = 1024 from the generator, and the restatement's answers for it (computed once, shared, never modified)"""
    if not BATCH:
        tokens, masks, kinds = dr.make_batch(1, 1024)
        BATCH.update(tokens=tokens, masks=masks, kinds=kinds, cap=(2048, 512, 1024))
        for strict in (False, True):
            BATCH[strict] = dr.decode_rows(tokens, masks, 2048, 512, 1024, strict)
        BATCH["split"] = [dr.split_and_restore(tokens[b], masks[b], 2048)[:3] for b in range(len(tokens))]
    return BATCH


def test_batch_composition_is_what_the_batch_test_needs():
    """on the CPU, from the restatement alone: the batch exercises what it is meant to"""
    bt = batch()
    assert bt["tokens"].shape == (96, 1024)
    loose, strict = bt[False], bt[True]
    assert sum(1 for r in strict if r["status"] == OK and len(r["notes"]) >= 16 and len(r["chords"]) >= 2) >= 32
    for branch in (0, 1, 2):
        assert sum(1 for r in strict if r["status"] == OK and r["branch"] == branch) >= 4, branch
    for st in (dr.NO_EOS, dr.RESTORE_FAILED, dr.ONCE_FAILED, dr.STRICT_FAILED, dr.REF_INDEXERROR, dr.BAD_META):
        assert sum(1 for r in strict if r["status"] == st) >= 8, st
    assert sum(1 for r in loose if r["status"] == OK and r["oov"] > 0) >= 4
    small = dr.decode_rows(bt["tokens"], bt["masks"], 160, 512, 1024)
    assert sum(1 for r in small if r["status"] == OVERFLOW) >= 1 and sum(1 for r in small if r["status"] == OK) >= 1


@pytest.mark.parametrize("strict", [False, True], ids=["once", "strict"])
def test_kernels_match_the_restatement_at_batch_scale(strict):
    test_batch_composition_is_what_the_batch_test_needs()
    bt = batch()
    split, out = run_kernels(bt["tokens"], bt["masks"], *bt["cap"], strict)
    check_against_rows(split, out, bt["split"], bt[strict], bt["cap"][0])


def test_overflow_from_small_capacities():
    bt = batch()
    for cap in ((160, 512, 1024), (2048, 20, 1024), (2048, 512, 6)):
        rows = dr.decode_rows(bt["tokens"], bt["masks"], *cap)
        assert any(r["status"] == OVERFLOW for r in rows) and any(r["status"] == OK for r in rows)
        split, out = run_kernels(bt["tokens"], bt["masks"], *cap, False)
        check_against_rows(split, out, [dr.split_and_restore(bt["tokens"][b], bt["masks"][b], cap[0])[:3] for b in range(96)], rows, cap[0])


def test_hostile_masks_end_in_a_status():
    """masks that are no 0 / 1 masks, all ones, all zeros, and rows of one repeated token: legal input, a status each"""
    bt = batch()
    tokens, masks = bt["tokens"][:24].copy(), bt["masks"][:24].copy()
    masks[0], masks[1], masks[2], masks[3] = 1, 0, 7, -1
    masks[4] = np.random.default_rng(0).integers(-2, 3, 1024)
    for k, t in enumerate((0, 1, 2, 432, 728, -5, 2 ** 31 - 1)):
        tokens[8 + k] = t
    tokens[16, 12:] = 2                                                                # Bars only behind the meta
    masks[17] = 1
    tokens[17] = 432                                                                   # len_meta 0 and a "chord part" of 432s: Bars to insert
    tokens[17, -1] = 1
    tempo0 = next(b for b in range(18, 24) if bt[False][b]["status"] == OK)
    tokens[tempo0, 0] = 560                                                            # bpm token of tempo 0: BAD_META (ours)
    rows = dr.decode_rows(tokens, masks, 2048, 512, 1024)
    assert {r["status"] for r in rows} >= {dr.BAD_META, dr.NO_EOS, dr.REF_INDEXERROR, OK} and rows[tempo0]["status"] == dr.BAD_META
    split, out = run_kernels(tokens, masks, 2048, 512, 1024, False)
    check_against_rows(split, out, [dr.split_and_restore(tokens[b], masks[b], 2048)[:3] for b in range(24)], rows, 2048)


def test_python_surface_and_controllability_on_device_rows():
    """split_meta_midi / decode_tokens wrap the same kernels; their device output feeds metric.Controllability_Pitch unchanged"""
    bt = batch()
    t, m = dev(bt["tokens"]), dev(bt["masks"])
    restored, lengths, meta, status = mdec.split_meta_midi(t, m)
    assert restored.shape == (96, 2048) and restored.is_cuda
    ref = bt["split"]
    assert np.array_equal(status.cpu().numpy(), [s[2] for s in ref])
    okr = np.array([s[2] == OK for s in ref])
    ref_rows = np.zeros((96, 2048), np.int32)
    for b, s in enumerate(ref):
        ref_rows[b, :len(s[0])] = s[0]
    ref_len, ref_meta = np.array([len(s[0]) for s in ref], np.int32), np.array([s[1] for s in ref], np.int32)
    assert np.array_equal(restored.cpu().numpy(), ref_rows) and np.array_equal(lengths.cpu().numpy(), ref_len)
    sel = torch.from_numpy(okr).to(DEV)
    got = metric.Controllability_Pitch(meta[sel], restored[sel], lengths[sel])
    want = metric.Controllability_Pitch(dev(ref_meta[okr]), dev(ref_rows[okr]), dev(ref_len[okr]))
    assert got == want and got[0] == int(okr.sum()) and 0 < got[1] < got[0]
    for strict in (False, True):
        rows = mdec.decode_tokens(t, m, strict_validation=strict).cpu()
        assert np.array_equal(rows.status, [r["status"] for r in bt[strict]])
        for b, r in enumerate(bt[strict]):
            assert tuple(rows.counts[b]) == tuple(r["counts"]) and np.array_equal(rows.notes[b], r["notes"]) and np.array_equal(rows.chords[b], r["chords"]), b


def test_decode_batch_end_to_end(tmp_path, capsys):
    """sampling.generate on the tiny golden model -> decode_batch, and decode_batch on device rows that do decode -> files"""
    from test_diffusion_gpu import build
    m, diff, _, inp, c = build("tiny")
    cond = {"input_ids": inp["batch"]["correct_ids"], "input_mask": inp["batch"]["input_mask"]}
    diff.noise_fn, diff.rng_mode = None, "philox"
    tok = sampling.generate(m, diff, cond, step=50)
    assert tok.is_cuda and tok.shape == (c["B"], c["L"])
    L = c["L"]
    rows = dr.decode_rows(tok.cpu().numpy(), cond["input_mask"].numpy(), 2 * L, 2 * L // 4 + 1, L + 1)     # decode_tokens' default capacities
    st = [r["status"] for r in rows]
    d0 = tmp_path / "tiny"
    d0.mkdir()
    if any(s in (dr.REF_INDEXERROR, dr.BAD_META, OVERFLOW) for s in st):                # 16-token rows of an untrained model: whatever they are,
        with pytest.raises((IndexError, KeyError, RuntimeError)):                       # decode_batch does with them what the restatement says
            mdec.decode_batch("generation", tok, cond["input_mask"], 0, 0, str(d0))
    else:
        bad = [i for i, s in enumerate(st) if s != OK]
        assert mdec.decode_batch("generation", tok, cond["input_mask"], 0, 0, str(d0), return_indices=True) == (len(st) - len(bad), bad)
        assert len(os.listdir(d0)) == len(st) - len(bad)
    keep = tuple(k for k in dr.BATCH_KINDS if k not in ("no_chords", "bad_meta"))[::4]
    tokens, masks, _ = dr.make_batch(5, 512, keep)
    for strict in (False, True):
        rows = dr.decode_rows(tokens, masks, 1024, 257, 513, strict)
        bad = [i for i, r in enumerate(rows) if r["status"] != OK]
        good = [i for i in range(len(rows)) if i not in bad]
        assert len(bad) >= 3 and len(good) >= 3
        gen, mod = tmp_path / ("gen%d" % strict), tmp_path / ("mod%d" % strict)
        gen.mkdir(), mod.mkdir()
        assert mdec.decode_batch("generation", dev(tokens).long(), dev(masks), 1, 10, str(gen), True, strict) == (len(good), bad)
        assert mdec.decode_batch("modification", torch.from_numpy(tokens), torch.from_numpy(masks), 3, 20, str(mod), strict_validation=strict) == len(good)
        assert sorted(os.listdir(gen)) == ["generated_%07d.midi" % (10 + k) for k in range(len(good))]
        assert sorted(os.listdir(mod)) == ["%07d_batch%05d_%04d.midi" % (20 + i, 3, i) for i in good]
        for k, i in enumerate(good):
            check_midi_file(str(gen / ("generated_%07d.midi" % (10 + k))), rows[i]["notes"], rows[i]["chords"], rows[i]["meta"])
            check_midi_file(str(mod / ("%07d_batch%05d_%04d.midi" % (20 + i, 3, i))), rows[i]["notes"], rows[i]["chords"], rows[i]["meta"])
    assert "Summary of Trial 1" in capsys.readouterr().out
