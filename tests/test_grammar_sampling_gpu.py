"""GPU: grammar-constrained rounding at the model level - sampling.generate / modify(constrained=True), model.argmax_tokens(constrain=),
run_generation / run_modification(constrained=True) - with the tiny random model of tests/test_infill_sampling_gpu.py.  The weights are
random, so the plain argmax of the last latent is noise the decoder rejects; the constrained rows decode.  With logits_mode 1 and these
weights some meta tokens do not come back from the argmax of their own embedding (tests/test_infill_sampling_gpu.py: the key 610), and
a row whose meta is not its own cannot be held to the decoder; with logits_mode 2 the anchored prefix comes back exactly and every
row is held."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import grammar_ref as gr  # noqa: E402
from gpu_helpers import library_launches  # noqa: E402
from musediffusion_amd import sampling  # noqa: E402
from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps  # noqa: E402
from musediffusion_amd.models.network import TransformerNetModel  # noqa: E402
from musediffusion_amd.utils import decode_util as du, grammar_util as gu  # noqa: E402
from oracle import denoiser as odn  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from test_grammar_gpu import int_tables  # noqa: E402

DEV = "cuda"
L, E, STEP, B = 128, 32, 4, 6


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
    g = np.random.default_rng(31)
    rows = [dr.make_row(g, L, "clean", n_bars=1 + b % 3, notes_per_bar=2) for b in range(B)]
    ids, mask = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    cond = {"input_ids": torch.from_numpy(ids).long(), "input_mask": torch.from_numpy(mask).long()}   # host tensors, as a loader hands them over
    gen = torch.Generator().manual_seed(5)
    noise = torch.randn(B, L, E, generator=gen)
    steps = [torch.randn(B, L, E, generator=gen) for _ in range(STEP)]
    diff.noise_fn = lambda k, i, x: steps[k].to(DEV)[:x.shape[0]]
    return mode, m, diff, cond, ids, mask, noise


def decodes(tokens, mask):
    return du.decode_tokens(tokens, torch.as_tensor(mask).to(DEV), strict_validation=True).status.cpu().numpy() == du.OK


@pytest.mark.parametrize("bars", ["exact", "decodable"])
def test_constrained_generate_decodes_where_the_plain_argmax_does_not(setup, bars):
    mode, m, diff, cond, ids, mask, noise = setup
    plain = sampling.generate(m, diff, cond, step=STEP, noise=noise, sharded=False)
    tok, res = sampling.generate(m, diff, cond, step=STEP, noise=noise, sharded=False, constrained=True, bars=bars)
    assert tok.dtype == torch.int64 and tok.shape == (B, L) and tok.is_cuda and isinstance(res, gu.ConstrainResult)
    t, p, st = tok.cpu().numpy(), plain.cpu().numpy(), res.status.cpu().numpy()
    prefix = mask == 0
    assert np.array_equal(t[prefix], p[prefix])                        # the anchored prefix is the plain run's
    assert (st == gu.CONSTRAIN_OK).all(), st
    own_meta = np.array([np.array_equal(p[b][prefix[b]][:-1], ids[b][prefix[b]][:-1]) for b in range(B)])
    if mode == 2:
        assert own_meta.all()
    assert own_meta.any()
    ok_plain, ok_con = decodes(plain, mask), decodes(tok, mask)
    print("GRAMMAR-SAMPLING mode %d bars %s: rows with their own meta %d / %d, plain decodes %d, constrained decodes %d" % (
        mode, bars, own_meta.sum(), B, ok_plain.sum(), ok_con.sum()))
    assert ok_con[own_meta].all(), (ok_con, own_meta)
    assert not ok_plain.all()                                          # at least one row of the plain run is lost
    counts = res.counts.cpu().numpy()
    n432 = np.array([(ids[b][11:int(prefix[b].sum()) - 1] == 432).sum() for b in range(B)])
    if bars == "exact":
        assert np.array_equal(counts[:, 0], n432)
    else:
        assert ((counts[:, 0] >= 0) & (counts[:, 0] <= n432 + 1)).all()
    for b in range(B):
        region = list(t[b][~prefix[b]])
        assert region.count(2) == counts[b, 0] and region.index(1) + 1 == counts[b, 2] and dr.validate_rigidly(region) == 1


def test_argmax_tokens_constrain_and_modify(setup):
    mode, m, diff, cond, ids, mask, noise = setup
    x = torch.randn(B, L, E, generator=torch.Generator().manual_seed(1)).to(DEV)
    plain = m.argmax_tokens(x)
    tok, res = m.argmax_tokens(x, constrain=(cond["input_ids"], cond["input_mask"]))
    seen = library_launches(lambda: m.argmax_tokens(x, constrain=(cond["input_ids"], cond["input_mask"])), strip="()")
    assert seen == ["class_argmax_kernel<%d>" % mode, "constrain_rows_kernel"], seen   # instead of the plain argmax, not after it
    t2, r2 = gu.constrain_tokens(m, x, cond["input_ids"], cond["input_mask"], "exact")
    assert torch.equal(tok, t2) and torch.equal(res.status, r2.status) and torch.equal(res.path_score, r2.path_score)
    cs, ci = gu.class_tables(m, x)
    assert torch.equal(ci[:, :, 7].long(), plain)
    want = gr.constrain_rows(cs.cpu().numpy(), ci.cpu().numpy(), ids, mask)
    assert np.array_equal(tok.cpu().numpy(), want["tokens"]) and np.array_equal(res.status.cpu().numpy(), want["status"])
    assert np.array_equal(res.path_score.cpu().numpy().view(np.int32), want["path_score"].view(np.int32))
    # modification mode: the same flag, per-row bounds as a tensor
    bars = torch.tensor([[1, 2]] * B)
    tok, res = sampling.modify(m, diff, cond, STEP, strength=0.5, noise=noise, sharded=False, constrained=True, bars=bars.to(DEV))
    c = res.counts.cpu().numpy()
    assert (res.status == gu.CONSTRAIN_OK).all() and ((c[:, 0] >= 1) & (c[:, 0] <= 2)).all()
    plain = sampling.modify(m, diff, cond, STEP, strength=0.5, noise=noise, sharded=False)
    assert torch.equal(tok[torch.as_tensor(mask == 0)], plain[torch.as_tensor(mask == 0)])


def stub_batch(g, ids, mask):
    """(tokens, ConstrainResult) as a constrained sampler returns them, from injected tables"""
    cs, ci = int_tables(g, len(ids), ids.shape[1], pad_bias=30)
    ci[:, :, 7] = np.where(mask == 0, ids, ci[:, :, 7])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    tokens, res = gu.constrain_rows(dev(cs, torch.float32), dev(ci, torch.int32), dev(ids, torch.int32), dev(mask, torch.int32), "exact")
    return tokens.long(), res


def test_run_generation_and_run_modification_constrained(setup):
    mode, m, diff, cond, ids, mask, noise = setup
    g = np.random.default_rng(3)
    meta, chord = dr.make_meta(g, 2, 1)
    # ---- generation with a stub sampler: the report, the log block, and nothing of it without the flag
    made = du.meta_to_batch(meta + chord, 4, L, DEV)
    mi, mm = made["input_ids"].cpu().numpy(), made["input_mask"].cpu().numpy()
    mi[1][mi[1] == 432] = 433                                          # a row whose meta names no bar: left as the plain argmax
    batches = [stub_batch(g, mi, mm) for _ in range(2)]
    logs = {True: [], False: []}
    it = iter(batches)
    rep = sampling.run_generation(None, None, meta + chord, batch_size=4, seq_len=L, num_samples=100, out_dir=None, max_batches=2,
                                  sampler=lambda cond: next(it), log=logs[True].append, device=DEV, constrained=True)
    assert rep.batches == 2 and rep.constrained["rows"] == dict(ok=6, bad_mask=0, no_chords=2, too_many_bars=0, bad_bounds=0, no_room=0, nonfinite=0)
    assert rep.constrained["bars"] == 12 and rep.constrained["notes"] == sum(int(r.counts[:, 1].sum()) for _, r in batches)
    assert rep.total_valid_count == 6
    assert sum("Grammar-constrained rounding: 6 of 8 rows" in s and "no_chords 2" in s for s in logs[True]) == 1
    it = iter(batches)
    seen = library_launches(lambda: logs.__setitem__("plain", sampling.run_generation(
        None, None, meta + chord, batch_size=4, seq_len=L, num_samples=100, out_dir=None, max_batches=2, sampler=lambda cond: next(it)[0],
        log=logs[False].append, device=DEV)), strip="()")
    plain = logs.pop("plain")
    assert not hasattr(plain, "constrained") and plain.total_valid_count == 6 and not any("Grammar" in s for s in logs[False])
    assert not [k for k in seen if "class_argmax" in k or "constrain_rows" in k]
    # ---- modification with a stub sampler
    it = iter(batches)
    loader = [{"input_ids": torch.from_numpy(mi).long(), "input_mask": torch.from_numpy(mm).long()}] * 2
    rep = sampling.run_modification(None, None, loader, step=STEP, batch_size=4, get_metric=False, sampler=lambda cond: next(it),
                                    log=lambda s: None, constrained=True)
    assert rep.constrained["rows"]["ok"] == 6 and rep.constrained["rows"]["no_chords"] == 2 and rep.total_valid_count == 6
    rep = sampling.run_modification(None, None, [], step=STEP, batch_size=4, log=lambda s: None, constrained=True)
    assert rep.constrained is None and rep.batches == 0
    # ---- one pass of each loop with the real sampler (not under the launch recorder: the reverse step is captured into a graph)
    rep = sampling.run_generation(m, diff, meta + chord, batch_size=2, seq_len=L, num_samples=1, step=STEP, out_dir=None, max_batches=1,
                                  log=lambda s: None, device=DEV, constrained=True, bars="decodable")
    assert rep.batches == 1 and rep.constrained["rows"]["ok"] == 2 and rep.constrained["notes"] >= 2
    rep = sampling.run_modification(m, diff, [cond], step=STEP, strength=0.5, batch_size=B, get_metric=False, log=lambda s: None, constrained=True)
    assert rep.batches == 1 and rep.constrained["rows"]["ok"] == B


def test_infill_refuses_constrained(setup):
    mode, m, diff, cond, ids, mask, noise = setup
    with pytest.raises(NotImplementedError, match="mid-row"):
        sampling.infill(m, diff, cond, (0, 1), step=STEP, constrained=True)
