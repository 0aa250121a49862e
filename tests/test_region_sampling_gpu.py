"""GPU: region rounding at the model level - sampling.infill / run_infill(rounding="region"), generate / modify(region=plan),
model.argmax_tokens(constrain=plan) - with the tiny random model and the pieces of tests/test_infill_sampling_gpu.py, in both logits
modes.  The weights are random, so the plain argmax of the region is noise of which the splice drops most; under the region rounding it
drops pads only.  What is pinned is the mechanics, not the music."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import infill_ref as ir  # noqa: E402
import region_ref as rr  # noqa: E402
from gpu_helpers import library_launches  # noqa: E402
from musediffusion_amd import sampling  # noqa: E402
from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps  # noqa: E402
from musediffusion_amd.models.network import TransformerNetModel  # noqa: E402
from musediffusion_amd.utils import decode_util as du, grammar_util as gu  # noqa: E402
from oracle import denoiser as odn  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from test_infill_sampling_gpu import BARS, KINDS, NOT_PLANNED, _bars_of, bars_tensor  # noqa: E402

DEV = "cuda"
L, E, STEP = 128, 32, 4
B = len(KINDS)


@pytest.fixture(scope="module", params=[1, 2])
def setup(request):
    mode = request.param
    c = dict(fx.CONFIGS["tiny"], L=L)
    sd = odn.random_state_dict(c["E"], c["H"], c["F"], c["nL"], c["V"], c["L"], c["Tt"], seed=fx.SEEDS["tiny"], emb_std=fx.EMB_STD)
    m = TransformerNetModel(c["E"], c["E"], c["Tt"], c["V"], c["L"], dropout=0.0, logits_mode=mode, bert_hidden=c["H"], bert_layers=c["nL"],
                            bert_heads=c["nh"], bert_ffn=c["F"], compute_dtype="fp32")
    m.load_state_dict(sd)
    m.eval().requires_grad_(False).to(DEV)
    diff = SpacedDiffusion(use_timesteps=space_timesteps(2000, [2000]), betas=get_named_beta_schedule("sqrt", 2000), rescale_timesteps=True,
                           predict_xstart=True)
    g = np.random.default_rng(22)
    rows = [dr.make_row(g, L, k, n_bars=3, notes_per_bar=3) for k in KINDS]
    tokens, mask = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    cond = {"input_ids": torch.from_numpy(tokens).long(), "input_mask": torch.from_numpy(mask).long()}     # host tensors, as a loader hands them over
    gen = torch.Generator().manual_seed(5)
    noise = torch.randn(B, L, E, generator=gen)
    steps = [torch.randn(B, L, E, generator=gen) for _ in range(STEP)]
    return mode, m, diff, cond, tokens, mask, noise, steps


def fixed_draws(diff, steps):
    diff.noise_fn = lambda k, i, x: steps[k].to(DEV)[:x.shape[0]]


def same_result(a, b):
    return torch.equal(a.status, b.status) and torch.equal(a.counts, b.counts) and torch.equal(a.path_score.view(torch.int32), b.path_score.view(torch.int32))


@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_region_infill_is_plan_sampler_splice_and_loses_nothing(setup, strength):
    mode, m, diff, cond, tokens, mask, noise, steps = setup
    fixed_draws(diff, steps)
    kw = dict(step=STEP, room=1, noise=noise, sharded=False, strength=strength)
    tok, res = sampling.infill(m, diff, cond, bars_tensor(), rounding="region", **kw)
    assert tok.dtype == torch.int64 and tok.shape == (B, L) and tok.is_cuda and isinstance(res.rounding, gu.RegionResult)
    # ---- composition, bit for bit
    plan = du.plan_infill(cond["input_ids"].to(DEV), cond["input_mask"].to(DEV), bars_tensor(), 1, "all")
    assert torch.equal(plan.tokens, res.plan.tokens) and torch.equal(plan.mask, res.plan.mask)
    plan_cond = {"input_ids": plan.tokens, "input_mask": plan.mask}
    if strength == 1:
        raw, rounded = sampling.generate(m, diff, plan_cond, step=STEP, noise=noise, sharded=False, region=plan)
        plain_raw = sampling.generate(m, diff, plan_cond, step=STEP, noise=noise, sharded=False)
    else:
        raw, rounded = sampling.modify(m, diff, plan_cond, step=STEP, strength=strength, noise=noise, sharded=False, region=plan)
        plain_raw = sampling.modify(m, diff, plan_cond, step=STEP, strength=strength, noise=noise, sharded=False)
    assert raw.dtype == torch.int64 and isinstance(rounded, gu.RegionResult) and same_result(rounded, res.rounding)
    spliced, counts = du.splice_infill(plan, raw)
    assert torch.equal(tok, spliced.long()) and torch.equal(res.counts, counts)
    # outside the mask the rounded sampler output is the plain run's, and so is every row that is not rounded
    outside = plan.mask != 1
    assert torch.equal(raw[outside], plain_raw[outside])
    st = rounded.status.cpu().numpy()
    assert st.tolist() == [gu.REGION_OK] * (B - 1) + [gu.REGION_NOT_PLANNED] and torch.equal(raw[NOT_PLANNED], plain_raw[NOT_PLANNED])
    # ---- the loss: on the same noise the plain run drops tokens of broken notes, the region run none
    plain_tok, plain = sampling.infill(m, diff, cond, bars_tensor(), **kw)
    assert plain.rounding is None and torch.equal(du.splice_infill(plan, plain_raw)[0].long(), plain_tok)
    pc, c, rc = plain.counts.cpu().numpy(), counts.cpu().numpy(), rounded.counts.cpu().numpy()
    print("REGION-SAMPLING mode %d strength %.1f: plain kept %d pads %d other %d | region kept %d pads %d other %d" % (
        mode, strength, pc[:, 0].sum(), pc[:, 1].sum(), pc[:, 2].sum(), c[:, 0].sum(), c[:, 1].sum(), c[:, 2].sum()))
    if strength == 1:
        assert pc[:, 2].sum() > 0                                      # the comparison is not vacuous: noise under random weights
    # (strength 0.5 of four steps re-noises the piece so little that the plain argmax returns it whole: there only the rest is held)
    ok = st == gu.REGION_OK
    assert not c[:, 2].any() and np.array_equal(c[ok, 0], 4 * rc[ok, 1]) and np.array_equal(c[ok, 1], rc[ok, 2])
    assert np.array_equal(rc[ok, 0], plan.info.cpu().numpy()[ok, 2]) and not rc[~ok].any() and not c[~ok].any()
    # ---- the kept parts: the piece up to the region, the kept notes between the region's BARs, the piece behind it, pads
    tok_h, info, ptok = tok.cpu().numpy(), plan.info.cpu().numpy(), plan.tokens.cpu().numpy()
    for b in range(B):
        lo, hi, n_mask, added = info[b]
        if b == NOT_PLANNED:
            assert np.array_equal(tok_h[b], tokens[b])
            continue
        kept = int(c[b, 0])
        assert np.array_equal(tok_h[b, :lo], tokens[b, :lo])
        rest = tokens[b, hi - added:L - added]
        n_bar = int((ptok[b, lo:hi] == ir.BAR).sum())
        inner = tok_h[b, lo:lo + kept + n_bar]
        assert (inner == ir.BAR).sum() == n_bar
        notes = inner[inner != ir.BAR]
        assert [ir.token_class(t) for t in notes] == [0, 1, 2, 3] * (kept // 4)
        after = lo + kept + n_bar
        assert np.array_equal(tok_h[b, after:after + len(rest)], rest) and not tok_h[b, after + len(rest):].any()


def test_the_result_decodes_strictly_and_the_other_bars_keep_their_notes(setup):
    mode, m, diff, cond, tokens, mask, noise, steps = setup
    fixed_draws(diff, steps)
    checked = 0
    for room in (2, 0):
        tok, res = sampling.infill(m, diff, cond, bars_tensor(), step=STEP, room=room, noise=noise, sharded=False, rounding="region")
        prefix = res.plan.prefix_mask
        assert torch.equal(prefix, cond["input_mask"].to(DEV).to(prefix.dtype))
        orig = du.decode_tokens(cond["input_ids"].to(DEV), prefix, strict_validation=True)
        got = du.decode_tokens(tok, prefix, strict_validation=True)
        o_rows, g_rows = orig.cpu(), got.cpu()
        tok_h = tok.cpu().numpy()
        for b, (lo, hi) in enumerate(BARS):
            if o_rows.status[b] != du.OK:
                continue
            # whole notes only, between the piece's own BARs: the strict validator passes; the decoder still wants one note in the row
            has_note = any(ir.token_class(t) == 1 for t in tok_h[b][mask[b] == 1])
            assert g_rows.status[b] == (du.OK if has_note else du.ONCE_FAILED), (room, b, g_rows.status[b])
            if g_rows.status[b] == du.OK:
                keep = lambda rows, dec: [tuple(int(x) for x in n) for n, k in zip(rows.notes[b], _bars_of(dec, b, rows.notes[b])) if not lo <= k < hi]  # noqa: E731
                assert keep(g_rows, got) == keep(o_rows, orig), (room, b)
                checked += 1
    assert checked >= 4                                                # rows 0 and 2 keep two bars of the piece's own notes, in both runs


def test_fields_pitch_rejects_nothing_and_changes_only_pitch_slots(setup):
    mode, m, diff, cond, tokens, mask, noise, steps = setup
    fixed_draws(diff, steps)
    tok, res = sampling.infill(m, diff, cond, bars_tensor(), step=STEP, fields="pitch", noise=noise, sharded=False, rounding="region")
    plain_tok, plain = sampling.infill(m, diff, cond, bars_tensor(), step=STEP, fields="pitch", noise=noise, sharded=False)
    tok_h, counts, rc = tok.cpu().numpy(), res.counts.cpu().numpy(), res.rounding.counts.cpu().numpy()
    pmask = res.plan.mask.cpu().numpy()
    assert res.plan.fields == 4 and pmask.sum(1).tolist() == [3, 3, 3, 3, 9, 0]
    assert not counts[:, 2].any() and counts[:, 0].tolist() == [3, 3, 3, 3, 9, 0]          # rejected 0: every selected slot taken
    print("REGION-SAMPLING mode %d fields=pitch: the plain run has %d of 21 slots rejected, the region run none" % (mode, int(plain.counts[:, 2].sum())))
    changed = tok_h != tokens
    assert (pmask[changed] == 1).all() and all(ir.token_class(t) == 2 for t in tok_h[pmask == 1]) and np.array_equal(changed.sum(1), counts[:, 3])
    assert res.rounding.status.tolist() == [gu.REGION_OK] * (B - 1) + [gu.REGION_NOT_PLANNED]
    assert rc[:, 0].tolist() == [3, 3, 3, 3, 9, 0] and not rc[:, 1:3].any() and rc[:, 3].tolist() == [3, 3, 3, 3, 9, 0]
    assert np.array_equal(tok_h[NOT_PLANNED], tokens[NOT_PLANNED])


def test_argmax_tokens_with_a_plan_and_the_mutual_exclusion(setup):
    mode, m, diff, cond, tokens, mask, noise, steps = setup
    plan = du.plan_infill(cond["input_ids"].to(DEV), cond["input_mask"].to(DEV), bars_tensor(), 1, "all")
    x = torch.randn(B, L, E, generator=torch.Generator().manual_seed(1)).to(DEV)
    plain = m.argmax_tokens(x)
    tok, res = m.argmax_tokens(x, constrain=plan)
    seen = library_launches(lambda: m.argmax_tokens(x, constrain=plan), strip="()")
    assert seen == ["class_argmax_kernel<%d>" % mode, "constrain_regions_kernel"], seen   # instead of the plain argmax, not after it
    t2, r2 = gu.constrain_region_tokens(m, x, plan)
    assert torch.equal(tok, t2) and same_result(res, r2) and tok.dtype == torch.int64
    cs, ci = gu.class_tables(m, x)
    assert torch.equal(ci[:, :, 7].long(), plain)
    want = rr.constrain_rows(cs.cpu().numpy(), ci.cpu().numpy(), plan.tokens.cpu().numpy(), plan.mask.cpu().numpy(), plan.status.cpu().numpy())
    assert np.array_equal(tok.cpu().numpy(), want["tokens"]) and np.array_equal(res.status.cpu().numpy(), want["status"])
    assert np.array_equal(res.path_score.cpu().numpy().view(np.int32), want["path_score"].view(np.int32))
    assert np.array_equal(res.counts.cpu().numpy(), want["counts"])
    outside = plan.mask != 1
    assert torch.equal(tok[outside], plain[outside]) and not torch.equal(tok, plain)
    # the tuple form is the row grammar's, unchanged
    t3, r3 = m.argmax_tokens(x, constrain=(cond["input_ids"], cond["input_mask"]))
    assert isinstance(r3, gu.ConstrainResult) and r3.counts.shape == (B, 3)
    plan_cond = {"input_ids": plan.tokens, "input_mask": plan.mask}
    with pytest.raises(ValueError, match="region"):
        sampling.generate(m, diff, plan_cond, step=STEP, sharded=False, region=plan, constrained=True)
    with pytest.raises(ValueError, match="region"):
        sampling.modify(m, diff, plan_cond, STEP, sharded=False, region=plan, constrained=True)
    with pytest.raises(ValueError, match="rounding"):
        sampling.infill(m, diff, cond, (0, 1), step=STEP, rounding="grammar")
    with pytest.raises(NotImplementedError, match="mid-row"):
        sampling.infill(m, diff, cond, (0, 1), step=STEP, constrained=True)
    with pytest.raises(NotImplementedError, match="mid-row"):
        sampling.infill(m, diff, cond, (0, 1), step=STEP, constrained=True, rounding="region")


def test_run_infill_with_region_rounding(setup, tmp_path, monkeypatch):
    mode, m, diff, cond, tokens, mask, noise, steps = setup
    diff.noise_fn, diff.rng_mode = None, "philox"
    corrupted = cond["input_ids"].clone()
    corrupted[corrupted == ir.EOS] = 0
    batch = {"input_ids": corrupted, "input_mask": cond["input_mask"], "correct_ids": cond["input_ids"]}
    loader = [batch, {k: v for k, v in batch.items() if k != "correct_ids"}]
    for where in (str(tmp_path / "out"), None):
        log = []
        rep = sampling.run_infill(m, diff, loader, bars=(0, 1), step=STEP, room=1, batch_size=B, out_dir=where, log=log.append, rounding="region")
        assert rep.batches == 2 and sum(rep.region["rows"].values()) == 2 * B
        # first batch: planned on correct_ids (five rows, one without EOS); second: on input_ids, whose EOS the corruption removed
        assert rep.region["rows"] == {"ok": 5, "not_planned": 1 + B, "bad_plan": 0, "nonfinite": 0, "no_room": 0}
        assert rep.infill["rows"]["ok"] == 5 and rep.infill["other"] == 0
        assert rep.infill["kept"] == 4 * rep.region["notes"] and rep.infill["pads"] == rep.region["pads"]
        assert rep.region["masked"] == rep.infill["kept"] + rep.infill["pads"] and rep.region["segments"] == 5
        assert sum(ln.startswith("### Region rounding:") for ln in log) == 1 and sum(ln.startswith("### Infill:") for ln in log) == 1
        if where:
            files = sorted(os.listdir(where))
            assert len(files) == rep.total_valid_count and all(f.endswith(".midi") for f in files)
    log = []
    rep = sampling.run_infill(m, diff, loader, bars=(0, 1), step=STEP, room=1, batch_size=B, out_dir=None, log=log.append)
    assert not hasattr(rep, "region") and not any("Region rounding" in ln for ln in log) and rep.infill["other"] > 0
    # ---- what the keyword adds to the loop: with the sampler stubbed (the reverse step is captured into a graph, which the launch
    # recorder cannot bracket) a run without the keyword launches the plan, the splice and the decode - nothing of the rounding -
    # and the run with it exactly one kernel more per batch
    g = np.random.default_rng(4)
    table = torch.from_numpy(g.integers(0, 729, (B, L))).to(DEV)
    calls = []

    def stub(model, diffusion, plan_cond, *a, region=None, **kw):
        calls.append(region is not None)
        if region is None:
            return table
        cs = torch.from_numpy(g.standard_normal((B, L, 8)).astype(np.float32)).to(DEV)
        ci = torch.from_numpy(g.integers(3, 131, (B, L, 8)).astype(np.int32)).to(DEV)
        tok, res = gu.constrain_regions(cs, ci, region)
        return tok.long(), res

    monkeypatch.setattr(sampling, "generate", stub)
    runs = {}
    for name, kw in (("plain", {}), ("argmax", {"rounding": "argmax"}), ("region", {"rounding": "region"})):
        box = []
        runs[name] = library_launches(lambda: box.append(sampling.run_infill(m, diff, loader, bars=(0, 1), step=STEP, room=1, batch_size=B,
                                                                              get_metric=False, log=lambda s: None, **kw)), strip="()")
        assert hasattr(box[0], "region") == (name == "region")
    assert calls == [False] * 4 + [True] * 2
    assert runs["plain"] == runs["argmax"] and runs["plain"][:2] == ["infill_plan_kernel", "infill_splice_kernel"]
    assert not [k for k in runs["plain"] if "constrain" in k or "class_argmax" in k]
    without = [k for k in runs["region"] if k != "constrain_regions_kernel"]
    assert without == runs["plain"] and len(runs["region"]) == len(runs["plain"]) + 2
