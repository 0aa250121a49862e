"""The optimizer matrix's bounds hold for plain float32 arithmetic, and its cases tell wrong kernels apart (CPU).

On the matrix's own inputs - the case lists of tests/test_optim_matrix_gpu.py, drawn by the generators of tests/optim_ref.py with the same
seeds - the float32 restatement of each kernel stays inside every bound (ratio at most 1.0: the AdamW bounds are worst-case and nearly
attained, so the whole bound is asked, not half of it; the measured peaks are printed).  Then each wrong variant below is judged by the
very function the GPU test asserts with (optim_ref.judge_adam / judge_norm / judge_clip) and must fail it in every case in which it
computes something else than the kernel - `applies` says in which and why.  A variant that stayed inside would get other inputs, not
another bound.

    no bias correction          b = 1 (steps up to 1000: at step 100000 sqrt(1 - 0.999^step) IS 1.0f; gradients of 1e-8 and above: at 1e-12
                                sqrt(v1) / b is 1e-4 of eps whatever b is), s = lr (steps 1 and 2: 1 - 0.9^1000 is 1 in double)
    eps inside the square root  sqrt(v1 + eps) / b; where v1 is not many orders above eps = 1e-8: gradients of 1e-4 and below, and the first
                                step at scale 1 (v1 = 1e-3 g^2 with zero moments: the |g| < 1e-2 elements).  With v1 of 0.01 to 1 (later steps
                                at scale 1) or 1e12 the two forms differ by less than the bound - by less than an ulp of p
    coupled L2 decay            g + wd p in place of p d; weight decay > 0
    EMA from the old p          gradient scales from 1e-8 up (below, p moves by less than an ulp of e and both are inside the bound)
    EMA skipped / moments decayed for NULL-gradient tensors
    norm                        the count % 4 tail dropped; one chunk dropped from the final sum
    clip                        without the 1e-6 (norms of 1e-4: at norms of 600 the 1e-6 is below half an ulp), scaling nothing, skipping tails"""
import numpy as np
import pytest

import optim_ref as orf
import test_optim_matrix_gpu as om

F = np.float32
LR = 1e-3


def _adam_case(case):
    table, nulls, n_ema, step, wd, gkind = case
    lay = orf.layout(table, nulls)
    return lay, orf.hparams(LR, wd, step, n_ema), orf.adam_inputs(lay, step, gkind, seed=step + n_ema)


def adam_outputs(lay, hp, inputs, variant=None):
    """the kernel's outputs in float32 numpy; variant: one of the wrong kernels"""
    p, g, m, v, e = inputs
    f = {k: hp[k] for k in hp}
    if variant == "no_bias2":
        f["bias2_sqrt"] = F(1)
    if variant == "no_bias1":
        f["step_size"] = F(LR)
    with orf.ignore():
        if variant == "eps_in_sqrt":
            m1 = m * f["beta1"] + g * f["one_minus_beta1"]
            v1 = v * f["beta2"] + (g * g) * f["one_minus_beta2"]
            p1 = p * f["decay_mul"] - f["step_size"] * (m1 / (np.sqrt(v1 + f["eps"]) / f["bias2_sqrt"]))
        elif variant == "coupled_l2":
            wd = F((1.0 - float(f["decay_mul"])) / LR)
            p1, m1, v1 = orf.adamw_restate(p, g + wd * p, m, v, dict(f, decay_mul=F(1)))
        else:
            p1, m1, v1 = orf.adamw_restate(p, g, m, v, f)
        live = lay.live
        if variant == "null_moments_decayed":
            m1, v1 = np.where(live, m1, m * f["beta1"]), np.where(live, v1, v * f["beta2"])
        else:
            m1, v1 = np.where(live, m1, m), np.where(live, v1, v)
        p1 = np.where(live, p1, p)
        es = []
        for k in range(hp["n_ema"]):
            e1 = orf.ema_restate(e[k], p if variant == "ema_old_p" else p1, hp["ema_rate"][k], hp["ema_one_minus"][k])
            es.append(np.where(live, e1, e[k]) if variant == "ema_skips_null" else e1)
    return p1.astype(F), m1.astype(F), v1.astype(F), es


def applies(variant, case, lay):
    table, nulls, n_ema, step, wd, gkind = case
    sc = orf.GSCALE[gkind]
    return {"no_bias2": step <= 1000 and sc >= 1e-8, "no_bias1": step <= 2, "eps_in_sqrt": sc <= 1e-4 or (sc == 1.0 and step == 1), "coupled_l2": wd > 0,
            "ema_old_p": n_ema > 0 and orf.GSCALE[gkind] >= 1e-8 and lay.live.any(), "ema_skips_null": n_ema > 0 and bool(lay.nulls),
            # (a NULL tensor of one element holds only the NaN half of its moment fill: NaN b1 is NaN)
            "null_moments_decayed": any(lay.sizes[t] > 1 for t in lay.nulls)}[variant]


ADAM_VARIANTS = ("no_bias2", "no_bias1", "eps_in_sqrt", "coupled_l2", "ema_old_p", "ema_skips_null", "null_moments_decayed")


@pytest.mark.parametrize("case", om.ADAM_CASES, ids=om._id)
def test_adamw_restatement_inside_the_bounds_and_wrong_variants_outside(case):
    lay, hp, inputs = _adam_case(case)
    got_p, got_m, got_v, got_e = adam_outputs(lay, hp, inputs)
    worst, share, fails = orf.judge_adam(lay, inputs, hp, got_p, got_m, got_v, got_e)
    print("OPTIM-BOUND adamw %s %s" % (om._id(case), " ".join("%s %.3f" % kv for kv in worst.items())))
    assert not fails and share == 1.0 and all(w <= 1.0 for w in worst.values()), fails
    for variant in ADAM_VARIANTS:
        if applies(variant, case, lay):
            _, _, fails = orf.judge_adam(lay, inputs, hp, *adam_outputs(lay, hp, inputs, variant))
            assert fails, "%s: the wrong variant %s passes every check" % (om._id(case), variant)


def test_every_adamw_variant_applies_somewhere():
    n = {v: sum(applies(v, c, orf.layout(c[0], c[1])) for c in om.ADAM_CASES) for v in ADAM_VARIANTS}
    assert all(k >= 3 for k in n.values()), n


def test_adamw_bounds_at_the_edges_of_the_derivation():
    """beyond the matrix's inputs: 1 M elements per setting with gradient scales 1e-22 to 1e6, zero g / m / v and m b1 = -g w1 (the
    specials of adam_inputs), steps 1 / 2 / 1000 / 100000; prints the peaks that profiles/optim_matrix.txt records"""
    lay = orf.Layout("flat", (1 << 18,), (), [(0, 1 << 18, 0)])
    peak = {}
    for step in (1, 2, 1000, 100000):
        for sc in (1e-22, 1e-16, 1e-12, 1e-8, 1e-4, 1.0, 1e6):
            inputs = orf.adam_inputs(lay, step, "s1", seed=step, scale=sc)
            hp = orf.hparams(LR, 0.01, step, 4)
            worst, share, fails = orf.judge_adam(lay, inputs, hp, *adam_outputs(lay, hp, inputs))
            assert not fails, (step, sc, fails)
            for k, w in worst.items():
                peak[k] = max(peak.get(k, 0.0), w)
    print("OPTIM-BOUND adamw edges " + " ".join("%s %.3f" % kv for kv in peak.items()))


# ------------------------------------------------------------------------------------------------------------------ norm
@pytest.mark.parametrize("case", om.NORM_CASES, ids=om._id)
def test_norm_restatement_inside_the_bounds_and_wrong_variants_outside(case):
    table, nulls, gkind = case
    lay = orf.layout(table, nulls)
    g = orf.norm_inputs(lay, gkind, seed=len(lay.chunks))
    part = orf.sumsq_restate(lay, g)
    wp, wn, fails = orf.judge_norm(lay, g, part, orf.norm_restate(part))
    print("OPTIM-BOUND norm %s partial %.3f norm %.3f depth %d" % (om._id(case), wp, wn, orf.total_depth(lay)))
    assert not fails and wp <= 1.0 and wn <= 1.0, fails
    if gkind in ("nan", "inf"):
        return
    tails = lay.tail_mask() & lay.live & (g != 0)
    if tails.any():
        short = orf.sumsq_restate(lay, g, drop_tail=True)
        assert orf.judge_norm(lay, g, short, orf.norm_restate(short))[2], "%s: the norm without the count %% 4 tails passes" % om._id(case)
    # one chunk dropped from the final sum (the heavy one where the case has it, else the table's largest, e.g. a 64 Ki one): told apart when
    # half its share of the sum of squares is twice the norm's relative bound or more.  It is not where every chunk has 8 elements of N(0, 1):
    # one of 50 000 is a 1e-5 of the sum, and a 196-deep fold of partials is allowed as much
    (pref, _), (nref, nb) = orf.sumsq_ref(lay, g)
    k = orf.heavy_chunk(lay) if gkind == "chunk" else int(np.argmax(pref))
    if lay.clive.sum() > 1 and pref[k] / pref.sum() / 2 > 2 * nb / nref:
        assert orf.judge_norm(lay, g, part, orf.norm_restate(part, skip=k))[2], "%s: the norm without chunk %d passes" % (om._id(case), k)
    else:
        # (a table of one chunk has none to lose; the 8-element table is what the "chunk" gradient set is for)
        assert lay.clive.sum() == 1 or (table == "c8" and gkind != "chunk"), "%s: cannot see a dropped chunk" % om._id(case)


def test_the_heavy_tail_and_heavy_chunk_carry_the_norm():
    for table, nulls, gkind in om.NORM_CASES:
        lay = orf.layout(table, nulls)
        g = orf.norm_inputs(lay, gkind, seed=len(lay.chunks)).astype(np.float64)
        g2 = np.where(lay.live, g, 0.0) ** 2
        if gkind == "tail":
            assert g2[lay.tail_mask()].sum() > 0.99 * g2.sum(), (table, nulls)
        if gkind == "chunk":
            assert g2[lay.chunk_mask(orf.heavy_chunk(lay))].sum() > 0.99 * g2.sum(), (table, nulls)


# ------------------------------------------------------------------------------------------------------------------ clip
def clip_variant(lay, g, norm, max_norm, variant):
    with orf.ignore():
        if variant == "no_eps":
            coef = np.minimum(F(1.0), F(max_norm) / F(norm))
        else:
            coef = orf.clip_coef(norm, max_norm)
        if coef >= 1.0 or variant == "scales_nothing":
            return g.copy()
        out = np.where(lay.live, g * coef, g).astype(F)
        if variant == "skips_tails":
            out = np.where(lay.tail_mask(), g, out)
        if variant == "fminf":                      # the kernel before this matrix: fminf(NaN, 1) = 1
            return g.copy() if np.isnan(coef) else out
    return out


@pytest.mark.parametrize("case", om.CLIP_CASES, ids=om._id)
def test_clip_prediction_and_wrong_variants(case):
    table, nulls, gkind, mode = case
    lay = orf.layout(table, nulls)
    g = orf.norm_inputs(lay, gkind, seed=len(lay.chunks))
    norm = orf.norm_restate(orf.sumsq_restate(lay, g))
    max_norm = om.clip_max_norm(mode, norm)
    want, coef = orf.clip_restate(lay, g, norm, max_norm)
    assert not orf.judge_clip(lay, g, norm, max_norm, clip_variant(lay, g, norm, max_norm, None))[1]
    if mode in ("below", "equal"):
        assert coef == 1.0 and orf.same_bits(want, g).all()
        return
    caught = lambda v: bool(orf.judge_clip(lay, g, norm, max_norm, clip_variant(lay, g, norm, max_norm, v))[1])
    assert caught("scales_nothing"), "a clip that scales nothing passes"
    if gkind == "nan":
        assert np.isnan(coef) and np.isnan(want[lay.live]).all() and orf.same_bits(want, g)[~lay.live].all() and caught("fminf")
        return
    if gkind == "inf":
        assert coef == 0.0 and np.isnan(want[lay.live]).sum() == 1 and (want[lay.live & np.isfinite(g)] == 0).all()
        return
    assert 0.0 < coef < 1.0 and (mode != "just_below" or coef >= 1.0 - 2 * orf.U)
    if (lay.tail_mask() & lay.live).any():
        assert caught("skips_tails"), "a clip that skips the count % 4 tails passes"
    if gkind == "small":
        assert caught("no_eps"), "a clip without the 1e-6 passes"


def test_clip_variants_are_exercised():
    """the cases that can show each clip variant exist: tails under a scaling coefficient, norms small enough for the 1e-6, a NaN norm"""
    small = [c for c in om.CLIP_CASES if c[2] == "small" and c[3] in ("above", "just_below")]
    assert len(small) >= 2 and {c[3] for c in small} == {"above", "just_below"}
    assert sum(c[2] == "nan" for c in om.CLIP_CASES) >= 2 and sum(c[2] == "inf" for c in om.CLIP_CASES) >= 2
    assert {c[3] for c in om.CLIP_CASES} >= {"above", "below", "equal", "just_below"}
