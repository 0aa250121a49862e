"""GPU: the two kernels of csrc/grammar.hip through the C ABI (include/musehip_grammar.h), outputs sentinel-filled between guard bands.
mhg_class_argmax against the float64 scores of tests/grammar_ref.py (slot 7 bit-equal to mh_logits_argmax / mh_distance_argmax, every
slot's score inside the per-element bound of its own index, every index within twice that bound of its class maximum, planted ties);
mhg_constrain_rows bit for bit against the restatement, on the kernel's own tables and on injected integer tables."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import distance_ref as dref  # noqa: E402
import grammar_ref as gr  # noqa: E402
from gpu_helpers import Guarded, library_launches  # noqa: E402
from musediffusion_amd import _lib, ops  # noqa: E402
from musediffusion_amd.utils import grammar_util as gu  # noqa: E402

DEV = "cuda"
SENT_F, SENT_I = 12345.0, -77
CUSTOM = ((0, 1), (1, 5), (5, 5), (60, 68), (68, 70), (80, 90), (-5, 3))    # V = 70: one empty, one across the 64-column seam, one outside V


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def classes_struct(classes):
    d = _lib.GrammarClasses()
    for c, (lo, hi) in enumerate(classes):
        d.lo[c], d.hi[c] = lo, hi
    return d


def run_class_argmax(x, W, aux, classes, mode):
    """-> (cls_score [n, 8], cls_idx [n, 8]) as numpy; x, W, aux are device tensors"""
    n, E, V = x.shape[0], x.shape[1], W.shape[0]
    cs, ci = Guarded(n, 8, dtype=torch.float32, sentinel=SENT_F), Guarded(n, 8)
    d = classes_struct(classes)
    _lib.check(_lib.lib().mhg_class_argmax(x.data_ptr(), W.data_ptr(), aux.data_ptr(), ctypes.byref(d), cs.ptr, ci.ptr, n, E, V, mode,
                                           _lib.current_stream()), "mhg_class_argmax")
    torch.cuda.synchronize()
    return cs.get(), ci.get()


def plain_argmax(x, W, aux, mode):
    n, E, V = x.shape[0], x.shape[1], W.shape[0]
    out = torch.full((n,), SENT_I, dtype=torch.int32, device=DEV)
    fn = _lib.lib().mh_logits_argmax if mode == 1 else _lib.lib().mh_distance_argmax
    _lib.check(fn(x.data_ptr(), W.data_ptr(), aux.data_ptr(), out.data_ptr(), n, E, V, _lib.current_stream()), "argmax")
    return out.cpu().numpy()


def score_inputs(V, E, n, mode, seed):
    """x [n, E], W [V, E], aux [V] (host) with duplicated table rows inside classes: an exact tie whose first index must win.  The pairs
    lie in one class, in different lanes and, the last, in different 64-row tiles."""
    g = np.random.default_rng(seed)
    W = (0.5 * g.standard_normal((V, E))).astype(np.float32)
    b = (0.3 * g.standard_normal(V)).astype(np.float32)
    pairs = ((135, 150), (440, 441), (10, 120), (310, 400)) if V == 729 else ((1, 3), (61, 66), (62, 67))
    for lo, hi in pairs:
        W[hi], b[hi] = W[lo], b[lo]
    x = (0.5 * g.standard_normal((n, E))).astype(np.float32)
    for k in range(0, n, 3):                                           # every third token sits next to a pair: mode 2's nearest, mode 1's longest dot
        lo = pairs[(k // 3) % len(pairs)][0]
        x[k] = (W[lo] * np.float32(4.0 if mode == 1 else 1.0) + np.float32(0.01) * g.standard_normal(E)).astype(np.float32)
    return x, W, b, pairs


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("E", [16, 100, 128])
@pytest.mark.parametrize("V", [729, 70])
def test_class_argmax_against_float64(V, E, mode):
    classes = gr.NOTE_CLASSES if V == 729 else CUSTOM
    worst_s = worst_i = 0.0
    tie_hits = 0
    for n in (1, 63, 64, 65, 130):
        x, W, b, pairs = score_inputs(V, E, n, mode, seed=V * 1000 + E * 10 + mode + n)
        xd, Wd = f32(x), f32(W)
        aux = f32(b) if mode == 1 else ops.row_sqnorm(Wd)
        got_s, got_i = run_class_argmax(xd, Wd, aux, classes, mode)
        # slot 7 is the existing entry point's answer bit for bit
        assert np.array_equal(got_i[:, 7], plain_argmax(xd, Wd, aux, mode)), (V, E, mode, n)
        if mode == 1:
            s64 = gr.scores64(x, W, b, 1)
            bound = (E + 2) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b).astype(np.float64)[None, :])
        else:
            s64, bound = dref.scores(x, W)[:2]                         # the bound tests/distance_ref.py derives for this expression
        want_s, want_i = gr.class_winners(s64, classes)
        rows = np.arange(n)
        for c in range(8):
            empty = want_i[:, c] < 0
            assert np.array_equal(got_i[:, c] < 0, empty), (V, E, mode, n, c)
            assert np.all(np.isneginf(got_s[empty, c])) and np.all(got_i[empty, c] == -1)
            live = ~empty
            if not live.any():
                continue
            lo, hi = (0, V) if c == 7 else (max(classes[c][0], 0), min(classes[c][1], V))
            idx = got_i[live, c]
            assert np.all((idx >= lo) & (idx < hi)), (V, E, mode, n, c)
            own, e = s64[rows[live], idx], bound[rows[live], idx]
            r_s = np.abs(got_s[live, c].astype(np.float64) - own) / e
            r_i = (want_s[live, c] - own) / (2 * e)
            worst_s, worst_i = max(worst_s, r_s.max()), max(worst_i, r_i.max())
            assert r_s.max() <= 1.0, "V=%d E=%d mode=%d n=%d slot %d: |score - float64| / bound = %.3f" % (V, E, mode, n, c, r_s.max())
            assert r_i.max() <= 1.0, "V=%d E=%d mode=%d n=%d slot %d: (class max - score of the index) / 2 bound = %.3f" % (V, E, mode, n, c, r_i.max())
            for first, second in pairs:                                 # the planted exact ties: never the later index
                assert not np.any(idx == second), (V, E, mode, n, c, second)
                tie_hits += int(np.sum(idx == first))
    print("GRAMMAR-CLASS-ARGMAX V=%d E=%d mode=%d  score %.3f  index %.3f of the bound, %d winners on a planted tie" % (V, E, mode, worst_s, worst_i, tie_hits))
    assert tie_hits > 0


def test_class_argmax_of_a_class_without_a_finite_score():
    g = np.random.default_rng(3)
    x, W = f32(g.standard_normal((5, 16))), f32(g.standard_normal((729, 16)))
    b = g.standard_normal(729).astype(np.float32)
    b[131:195] = -np.inf
    b[2] = np.nan
    cs, ci = run_class_argmax(x, W, f32(b), gr.NOTE_CLASSES, 1)
    for c in (gr.VELOCITY, gr.BAR):                                    # all -inf, all NaN: nothing ever wins
        assert np.all(ci[:, c] == -1) and np.all(np.isneginf(cs[:, c]))
    assert np.all(ci[:, gr.PITCH] >= 3) and np.all(np.isfinite(cs[:, gr.PITCH]))


# ------------------------------------------------------------------------------------------------------------------ the row Viterbi
def run_constrain(cs, ci, ids, mask, lo=None, hi=None, policy=gr.BARS_EXACT):
    """mhg_constrain_rows through the C ABI -> dict of numpy arrays, as grammar_ref.constrain_rows; cs / ci [B, L, 8] host or device"""
    B, L = ids.shape
    csd = cs if isinstance(cs, torch.Tensor) else f32(cs)
    cid = ci if isinstance(ci, torch.Tensor) else i32(ci)
    idd, md = i32(ids), i32(mask)
    lod, hid = (None, None) if lo is None else (i32(lo), i32(hi))
    out = dict(tokens=Guarded(B, L), status=Guarded(B), path_score=Guarded(B, dtype=torch.float32, sentinel=SENT_F), counts=Guarded(B, 3))
    _lib.check(_lib.lib().mhg_constrain_rows(csd.data_ptr(), cid.data_ptr(), idd.data_ptr(), md.data_ptr(), None if lod is None else lod.data_ptr(),
                                             None if hid is None else hid.data_ptr(), policy, out["tokens"].ptr, out["status"].ptr,
                                             out["path_score"].ptr, out["counts"].ptr, None, 0, B, L, _lib.current_stream()), "mhg_constrain_rows")
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}


def same(got, want, what=""):
    for name in ("status", "counts", "tokens"):
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist(), got["status"][:8], want["status"][:8])
    assert np.array_equal(got["path_score"].view(np.int32), want["path_score"].view(np.int32)), (what, got["path_score"][:4], want["path_score"][:4])


def check(cs, ci, ids, mask, lo=None, hi=None, policy=gr.BARS_EXACT, what=""):
    got = run_constrain(cs, ci, ids, mask, lo, hi, policy)
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t  # noqa: E731
    want = gr.constrain_rows(host(cs), host(ci), ids, mask, policy, lo, hi)
    same(got, want, what)
    return got


def int_tables(g, B, L, pad_bias=0):
    """integer scores in [-64, 64] and per-slot indices in the ComMU classes; slot 7 is junk of its own (a token the grammar never emits)"""
    cs = g.integers(-64, 65, (B, L, 8)).astype(np.float32)
    cs[:, :, gr.PAD] += pad_bias
    ci = np.zeros((B, L, 8), np.int32)
    for c, (lo, hi) in enumerate(gr.NOTE_CLASSES):
        ci[:, :, c] = g.integers(lo, hi, (B, L))
    ci[:, :, 7] = g.integers(560, 729, (B, L))
    return cs, ci


def masks(B, L, len_meta):
    """ids / mask [B, L] with the given len_meta per row (ids: junk without a 432; the bounds come from the caller)"""
    lm = np.broadcast_to(np.asarray(len_meta), (B,))
    mask = (np.arange(L)[None, :] >= lm[:, None]).astype(np.int32)
    return np.full((B, L), 600, np.int32), mask


@pytest.mark.parametrize("L,B,his", [(64, 1, (0, 1, 16)), (65, 2, (0, 1, 16, 63)), (256, 2, (0, 16, 63)), (257, 65, (1, 63)), (64, 65, (0, 16)),
                                     (4096, 1, (63,)), (4096, 2, (16,))])
def test_constrain_rows_on_injected_integer_tables(L, B, his):
    g = np.random.default_rng(L * 100 + B)
    for hi in his:
        for pad_bias in (0, 40):
            cs, ci = int_tables(g, B, L, pad_bias)
            len_meta = g.integers(0, max(1, L - (hi + 5)), B)            # the region has room for hi Bars, a note and the EOS
            ids, mask = masks(B, L, len_meta)
            lo = np.minimum(g.integers(0, hi + 1, B), L - len_meta - 5).astype(np.int32)   # lo Bars, a note and the EOS fit
            got = check(cs, ci, ids, mask, lo, np.full(B, hi, np.int32), what="L=%d B=%d hi=%d bias=%d" % (L, B, hi, pad_bias))
            assert (got["status"] == gr.OK).all()
            assert (got["counts"][:, 0] >= lo).all() and (got["counts"][:, 0] <= hi).all()
            if L <= 257:                                                # and the rows are what the decoder's validator walks to the EOS
                for b in range(min(B, 3)):
                    assert dr.validate_rigidly(list(got["tokens"][b, len_meta[b]:])) == 1


def test_4097_tokens_and_64_bars():
    g = np.random.default_rng(2)
    cs, ci = int_tables(g, 1, 128)
    ids, mask = masks(1, 128, 20)
    got = check(cs, ci, ids, mask, np.array([0]), np.array([64]))
    assert got["status"][0] == gr.TOO_MANY_BARS and np.array_equal(got["tokens"][0], ci[0, :, 7])
    a = torch.zeros(8, dtype=torch.int32, device=DEV).data_ptr()
    assert _lib.lib().mhg_constrain_rows(a, a, a, a, None, None, 0, a, a, a, a, None, 0, 1, 4097, None) == _lib.MH_ERR_INVALID
    with pytest.raises(ValueError):
        gu.constrain_rows(torch.zeros(1, 4097, 8, device=DEV), torch.zeros(1, 4097, 8, device=DEV, dtype=torch.int32),
                          torch.zeros(1, 4097, device=DEV, dtype=torch.int32), torch.ones(1, 4097, device=DEV, dtype=torch.int32))


def test_edges_forced_eos_exact_room_neg_inf_and_nan():
    g = np.random.default_rng(4)
    L, lm = 96, 30
    n = L - lm
    ids, mask = masks(1, L, lm)
    cs, ci = int_tables(g, 1, L)
    for lo in (0, 3):
        last = lo + 4 * ((n - 1 - lo) // 4)                             # lo Bars and whole notes in front of it
        for at in (lo + 4, last):                                       # the first and the last legal place of the EOS
            hot = cs.copy()
            hot[0, lm + at, gr.EOS] = 1.0e6
            got = check(hot, ci, ids, mask, np.array([lo]), np.array([lo]), what="eos at %d" % at)
            assert got["status"][0] == gr.OK and got["counts"][0, 2] == at + 1 and got["tokens"][0, lm + at] == 1
    for lo in (0, 1, 63):                                               # a region of exactly lo + 5, and one token less
        ids2, mask2 = masks(1, L, L - (lo + 5))
        got = check(cs, ci, ids2, mask2, np.array([lo]), np.array([63]), what="exact room")
        assert got["status"][0] == gr.OK and tuple(got["counts"][0]) == (lo, 1, lo + 5)
        ids2, mask2 = masks(1, L, L - (lo + 4))
        assert check(cs, ci, ids2, mask2, np.array([lo]), np.array([63]))["status"][0] == gr.NO_ROOM
    # -inf: one class at every position, every class at one position, a class without a token
    for c in range(7):
        cold = cs.copy()
        cold[0, :, c] = -np.inf
        got = check(cold, ci, ids, mask, np.array([1]), np.array([4]), what="-inf class %d" % c)
        assert got["status"][0] == gr.OK
        gone = ci.copy()
        gone[0, :, c] = -1
        got = check(cs, gone, ids, mask, np.array([0]), np.array([4]), what="class %d without a token" % c)
        assert got["status"][0] == (gr.OK if c in (gr.PAD, gr.BAR) else gr.NO_ROOM)
    cold = cs.copy()
    cold[0, lm + 7, :7] = -np.inf
    got = check(cold, ci, ids, mask, np.array([1]), np.array([4]), what="-inf position")
    assert got["status"][0] == gr.OK and np.isneginf(got["path_score"][0])
    # NaN or +inf at one position of the region is a status; outside the region and in slot 7 nothing is looked at
    for bad in (np.nan, np.inf):
        for pos, slot, st in ((lm, 0, gr.NONFINITE), (L - 1, 6, gr.NONFINITE), (lm + 64, 3, gr.NONFINITE), (lm - 1, 2, gr.OK), (lm + 5, 7, gr.OK)):
            hot = cs.copy()
            hot[0, pos, slot] = bad
            got = check(hot, ci, ids, mask, np.array([1]), np.array([4]), what="nonfinite")
            assert got["status"][0] == st


def status_batch(g, L=128):
    """rows of every status next to rows that are OK -> cs, ci, ids, mask, lo, hi, the statuses expected"""
    kinds = ["ok", "bad_mask", "ok", "too_many", "bad_bounds", "no_room", "nonfinite", "ok", "bad_mask_all", "lo_above_hi", "ok"]
    B = len(kinds)
    cs, ci = int_tables(g, B, L)
    ids, mask = masks(B, L, 40)
    lo, hi = np.full(B, 1, np.int32), np.full(B, 5, np.int32)
    for b, k in enumerate(kinds):
        if k == "bad_mask":
            mask[b] = 0
        elif k == "bad_mask_all":
            mask[b] = 3
        elif k == "too_many":
            hi[b] = 64
        elif k == "bad_bounds":
            lo[b] = -1
        elif k == "lo_above_hi":
            lo[b] = 6
        elif k == "no_room":
            mask[b] = (np.arange(L) >= L - 5).astype(np.int32)
        elif k == "nonfinite":
            cs[b, 77, gr.PITCH] = np.nan
    want = {"ok": gr.OK, "bad_mask": gr.BAD_MASK, "bad_mask_all": gr.BAD_MASK, "too_many": gr.TOO_MANY_BARS, "bad_bounds": gr.BAD_BOUNDS,
            "lo_above_hi": gr.BAD_BOUNDS, "no_room": gr.NO_ROOM, "nonfinite": gr.NONFINITE}
    return cs, ci, ids, mask, lo, hi, np.array([want[k] for k in kinds], np.int32)


def test_every_status_inside_one_batch_and_repeated_bits():
    g = np.random.default_rng(6)
    cs, ci, ids, mask, lo, hi, want = status_batch(g)
    first = check(cs, ci, ids, mask, lo, hi, what="explicit bounds")
    assert np.array_equal(first["status"], want)
    bad = first["status"] != gr.OK
    assert np.array_equal(first["tokens"][bad], ci[bad][:, :, 7]) and not first["counts"][bad].any() and not first["path_score"][bad].any()
    again = run_constrain(cs, ci, ids, mask, lo, hi)
    same(again, first, "repeat")
    # the policies that ask the meta: NO_CHORDS beside rows that are OK
    rows = [dr.make_row(g, 160, "clean", n_bars=nb, notes_per_bar=2) for nb in (1, 3, 8, 2)]
    ids2, mask2 = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    ids2[1][ids2[1] == 432] = 433
    cs2, ci2 = int_tables(g, 4, 160, pad_bias=30)
    for policy in (gr.BARS_EXACT, gr.BARS_DECODABLE):
        got = check(cs2, ci2, ids2, mask2, policy=policy, what="policy %d" % policy)
        assert got["status"].tolist() == [gr.OK, gr.NO_CHORDS, gr.OK, gr.OK]
        if policy == gr.BARS_EXACT:
            assert got["counts"][:, 0].tolist() == [1, 0, 8, 2]


def test_constrain_rows_on_the_kernels_own_tables_decodes():
    """class winners of random hidden states against a random table, rows with ComMU metas: the tables never leave the device, the
    restatement reads a copy, and every constrained row passes the decode restatement with the strict validator"""
    g = np.random.default_rng(7)
    B, L, E, V = 6, 192, 32, 729
    rows = [dr.make_row(g, L, "clean", n_bars=1 + b, notes_per_bar=2) for b in range(B)]
    ids, mask = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    W = f32(0.5 * g.standard_normal((V, E)))
    x = 0.5 * g.standard_normal((B, L, E))
    x[mask == 0] = W.cpu().numpy()[ids[mask == 0]] * 8                 # the anchored prefix scores its own token highest (mode 1: a long dot)
    bias = np.zeros(V, np.float32)
    bias[0] = 3.0                                                      # a head that likes PAD, as a trained one does behind the EOS
    for mode, aux in ((1, f32(bias)), (2, ops.row_sqnorm(W))):
        xs = f32(x if mode == 1 else np.where((mask == 0)[:, :, None], x / 8, x))
        cs, ci = ops.class_argmax(xs, W, aux, mode)
        cs, ci = cs.view(B, L, 8), ci.view(B, L, 8)
        plain = ci[:, :, 7].cpu().numpy()
        assert np.array_equal(plain[mask == 0], ids[mask == 0])
        for policy in (gr.BARS_EXACT, gr.BARS_DECODABLE):
            got = check(cs, ci, ids, mask, policy=policy, what="own tables, mode %d policy %d" % (mode, policy))
            assert (got["status"] == gr.OK).all()
            for b in range(B):
                assert dr.decode_row(got["tokens"][b], mask[b], 2 * L, L, L, strict=True)["status"] == dr.OK
                assert dr.decode_row(plain[b], mask[b], 2 * L, L, L, strict=True)["status"] != dr.OK


# ------------------------------------------------------------------------------------------------------------------ the Python front
@pytest.mark.parametrize("mode", [1, 2])
def test_constrain_tokens_is_two_launches_whatever_the_batch(mode):
    g = np.random.default_rng(9)
    V, E, L = 729, 16, 96
    W = torch.nn.Parameter(f32(0.5 * g.standard_normal((V, E))), requires_grad=False)
    head = SimpleNamespace(weight=W, bias=f32(np.zeros(V)))
    norms = ops.row_sqnorm(W)
    model = SimpleNamespace(logits_mode=mode, lm_head=head, word_embedding=SimpleNamespace(weight=W), embedding_norms=lambda: norms)
    for B in (2, 64):
        ids, mask = masks(B, L, 30)
        x = f32(g.standard_normal((B, L, E)))
        box = []
        bars = torch.tensor([[1, 4]] * B, device=DEV)
        seen = library_launches(lambda: box.append(gu.constrain_tokens(model, x, i32(ids).long(), i32(mask).long(), bars)), strip="()")
        assert seen == ["class_argmax_kernel<%d>" % mode, "constrain_rows_kernel"], seen
        tokens, res = box[0]
        assert tokens.dtype == torch.int64 and tokens.shape == (B, L) and res.status.shape == (B,) and res.counts.shape == (B, 3)
        cs, ci = gu.class_tables(model, x)
        want = gr.constrain_rows(cs.cpu().numpy(), ci.cpu().numpy(), ids, mask, lo=[1] * B, hi=[4] * B)
        same(dict(tokens=tokens.cpu().numpy().astype(np.int32), status=res.status.cpu().numpy(), path_score=res.path_score.cpu().numpy(),
                  counts=res.counts.cpu().numpy()), want, "front")
        for spec in ((1, 4), "exact", "decodable"):
            t2, r2 = gu.constrain_tokens(model, x, i32(ids), i32(mask), spec)
            if spec == (1, 4):
                assert torch.equal(t2, tokens) and torch.equal(r2.status, res.status)
            else:
                assert (r2.status == gu.CONSTRAIN_NO_CHORDS).all() and torch.equal(t2, ci[:, :, 7].long())
        s = res.summary()
        assert s["rows"]["ok"] == B and s["bars"] == int(res.counts[:, 0].sum()) and s["notes"] == int(res.counts[:, 1].sum())
    with pytest.raises(ValueError):
        gu.constrain_tokens(model, x, i32(ids), i32(mask), "loose")
