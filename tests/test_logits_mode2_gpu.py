"""logits_mode 2 end to end (GPU): a TransformerNetModel built with logits_mode=2 trains both NLL terms of training_losses on, and decodes
its samples with, the distance logits of get_logits (network.py:94-104) - as the reference, which routes both through get_logits
(diffusion.py:556-575, run/sample.py:219-220).  All at the `tiny` fixture shape in fp32 mode, against the CPU oracle (torch autograd over
the restated reference ops, pinned to the reference's own mode-2 output by tests/test_oracle_golden.py).

Tolerances of the losses test: tests/test_training_gpu.py::test_every_parameter_gradient_matches_oracle's - 5e-4 of the losses' max-abs,
2e-3 of each gradient's max-abs (+ 1e-7).  Measured on an MI355X: see the docstring of the test."""
import numpy as np
import pytest
import torch

import distance_ref as dr

pytestmark = pytest.mark.gpu

from conftest import load_golden  # noqa: E402
from musediffusion_amd import sampling  # noqa: E402
from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps  # noqa: E402
from musediffusion_amd.models.network import TransformerNetModel  # noqa: E402
from musediffusion_amd.train_step import TrainStep  # noqa: E402
from oracle import denoiser as odn, fixtures as fx, losses as olo, schedule as osc  # noqa: E402
from test_diffusion_gpu import loop_noises  # noqa: E402
from test_training_gpu import CpuDraws, close  # noqa: E402

DEV = "cuda"
TAG = "tiny"


def build(logits_mode, train):
    c = fx.CONFIGS[TAG]
    m = TransformerNetModel(c["E"], c["E"], c["Tt"], c["V"], c["L"], dropout=0.0, logits_mode=logits_mode, bert_hidden=c["H"],
                            bert_layers=c["nL"], bert_heads=c["nh"], bert_ffn=c["F"], compute_dtype="fp32", bert_hidden_dropout=0.0,
                            bert_attention_dropout=0.0)
    m.load_state_dict(fx.state_dict(TAG))
    if train:
        m.train().requires_grad_(True).to(DEV)
    else:
        m.eval().requires_grad_(False).to(DEV)
    diff = SpacedDiffusion(use_timesteps=space_timesteps(2000, [2000]), betas=get_named_beta_schedule("sqrt", 2000),
                           rescale_timesteps=True, predict_xstart=True)
    return m, diff, c


def run_losses(m, diff, variant):
    li = fx.loss_inputs(TAG)
    batch, t, w = li["batch"], li["t"], li["w"]
    kw = {k: v for k, v in batch.items() if variant == "corrupt" or k != "correct_ids"}
    with CpuDraws(fx.loss_seed(TAG)):
        terms = diff.training_losses(m, t.to(DEV), model_kwargs=kw)
    return terms, batch, t, w


def oracle_losses(variant, batch, t, w):
    """oracle.losses.training_losses with the mode-2 logits under torch autograd, lm_head.weight tied; -> terms, {name: grad}"""
    c = fx.CONFIGS[TAG]
    sd = {k: v.clone() for k, v in fx.state_dict(TAG).items()}
    names = [n for n in sd if n != "lm_head.weight" and sd[n].is_floating_point()]
    for n in names:
        sd[n].requires_grad_(True)
    sd["lm_head.weight"] = sd["word_embedding.weight"]
    g = torch.Generator().manual_seed(fx.loss_seed(TAG))
    shape = (c["B"], c["L"], c["E"])
    draws = {"x_start": torch.randn(shape, generator=g, dtype=torch.float32)}
    if variant == "corrupt":
        draws["correct"] = torch.randn(shape, generator=g, dtype=torch.float32)
    draws["noise"] = torch.randn(shape, generator=g, dtype=torch.float32)
    d = osc.make_diffusion()
    ref = olo.training_losses(d, lambda x, ts: odn.forward(sd, x, ts, c["nh"]), lambda ids: odn.get_embeds(sd, ids),
                              lambda h: odn.get_logits(sd, h, logits_mode=2), t, batch["input_ids"], batch["input_mask"],
                              correct_ids=batch["correct_ids"] if variant == "corrupt" else None, draws=draws)
    (ref["loss"] * w).mean().backward()
    return ref, {n: sd[n].grad for n in names}


@pytest.mark.parametrize("variant", ["plain", "corrupt"])
def test_mode2_training_losses_and_every_gradient_match_the_oracle(variant):
    """mse, nll, loss and EVERY parameter's gradient of training_losses on a logits_mode=2 model against the oracle's, same draws.
    lm_head.bias takes no part: its gradient is None on both sides.
    Measured on an MI355X (both variants): mse / nll / loss within 7.2e-7 absolute (tolerance 5e-4 of max-abs = 1.9e-3 ... 3.4e-3); the
    worst gradient is word_embedding.weight's at 2.1e-6 of its max-abs, every other one below 6e-7 (tolerance 2e-3): the tolerances of
    test_every_parameter_gradient_matches_oracle fit mode 2 as they stand."""
    m, diff, c = build(2, train=True)
    terms, batch, t, w = run_losses(m, diff, variant)
    (terms["loss"] * w.to(DEV)).mean().backward()
    ref, rgrads = oracle_losses(variant, batch, t, w)
    for k in ("mse", "nll", "loss"):
        close("%s %s" % (variant, k), terms[k], ref[k].detach().numpy(), 5e-4)
    assert m.lm_head.bias.grad is None and rgrads["lm_head.bias"] is None
    bad = []
    for n, p in m.named_parameters():
        if n == "lm_head.bias":
            continue
        r = rgrads[n]
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        err = float((p.grad.detach().cpu() - r).abs().max())
        scale = float(r.abs().max())
        print("%s grad %s: max abs err %.3e (ref absmax %.3e, ratio %.2e)" % (variant, n, err, scale, err / (scale + 1e-30)))
        # key biases have a zero true gradient (softmax is invariant to a per-query shift): only rounding noise on both sides
        if "attention.self.key.bias" in n:
            assert err < 1e-5, (n, err)
            continue
        if err > 2e-3 * scale + 1e-7:
            bad.append((n, err, scale))
    assert not bad, bad


def test_mode2_nll_is_not_the_mode1_nll():
    """the dispatch guard: the same call on a mode-1 model with the same weights gives another nll (and another loss through the decoder
    term) by more than the losses test's tolerance on every sequence (measured: |d nll| >= 0.026 against 5e-4 x 6.68 = 0.0033), while
    mse - which no logits enter - is the same bit for bit"""
    m2, diff, _ = build(2, train=True)
    m1, _, _ = build(1, train=True)
    with torch.no_grad():
        t2 = run_losses(m2, diff, "plain")[0]
        t1 = run_losses(m1, diff, "plain")[0]
    assert torch.equal(t1["mse"], t2["mse"])
    for k in ("nll", "loss"):
        d = float((t1[k] - t2[k]).abs().min())
        print("mode 1 vs mode 2 %s: min |difference| %.4f" % (k, d))
        assert d > 5e-4 * float(t2[k].abs().max()), (k, d)


def _positions():
    """rows of the golden mode-2 file's `hidden` (random positions and exact table rows) and the golden ddim50 loop's final sample"""
    h = np.asarray(load_golden("logits_mode2.npz")["hidden"]).reshape(-1, fx.CONFIGS[TAG]["E"])
    s = np.asarray(load_golden("model_%s.npz" % TAG)["loop_ddim50"]).reshape(-1, fx.CONFIGS[TAG]["E"])
    return np.concatenate([h, s]).astype(np.float32)


def test_mode2_argmax_tokens_is_the_argmax_of_get_logits_and_of_the_oracle():
    m, _, c = build(2, train=False)
    x = _positions()
    W = fx.state_dict(TAG)["lm_head.weight"].numpy()
    bound = dr.scores(x, W)[1].max(1)                                   # the row's largest score bound (tests/distance_ref.py)
    xd = torch.from_numpy(x).to(DEV).view(1, -1, c["E"])
    logits = m.get_logits(xd)[0].cpu()
    top2 = logits.topk(2, dim=-1).values
    safe = (top2[:, 0] - top2[:, 1]).numpy() > bound
    assert int((~safe).sum()) <= 0.01 * len(safe)
    tok = m.argmax_tokens(xd)
    assert tok.dtype == torch.int64 and tok.shape == (1, len(x))
    tok = tok[0].cpu().numpy()
    assert np.array_equal(tok[safe], logits.argmax(-1).numpy()[safe])
    ref = odn.get_logits(fx.state_dict(TAG), torch.from_numpy(x).view(1, -1, c["E"]), logits_mode=2)[0].argmax(-1).numpy()
    assert np.array_equal(tok[safe], ref[safe])
    # not what mode 1 decodes: lm_head(x) + bias ranks the rows differently
    m1, _, _ = build(1, train=False)
    assert not np.array_equal(m1.argmax_tokens(xd)[0].cpu().numpy(), tok)


def test_mode2_argmax_follows_the_weights():
    """the |W_v|^2 cache of embedding_norms() is refreshed with the engine when the table changes in place (as an optimizer step does)"""
    m, _, c = build(2, train=False)
    x = torch.from_numpy(_positions()).to(DEV).view(1, -1, c["E"])
    before = m.argmax_tokens(x)
    with torch.no_grad():
        m.word_embedding.weight[::2] *= 3.0
    after = m.argmax_tokens(x)
    top2 = m.get_logits(x).topk(2, dim=-1).values
    bound = torch.from_numpy(dr.scores(_positions(), m.lm_head.weight.detach().cpu().numpy())[1].max(1)).to(DEV).view(1, -1)
    safe = (top2[..., 0] - top2[..., 1]).double() > bound
    assert bool(safe.all())
    assert torch.equal(after[safe], m.get_logits(x).argmax(-1)[safe]) and not torch.equal(before, after)


def test_mode2_generate_decodes_with_the_distance_logits():
    """sampling.generate on a mode-2 model: the reverse loop does not depend on the logits mode, so its final sample is the golden loop's;
    the tokens are the argmax of the ORACLE's mode-2 logits of that sample, on the margin rule of the argmax test"""
    m, diff, c = build(2, train=False)
    sd = fx.state_dict(TAG)
    inp = fx.case_inputs(TAG, sd["word_embedding.weight"])
    B, L, E = c["B"], c["L"], c["E"]
    cond = {"input_ids": inp["batch"]["correct_ids"], "input_mask": inp["batch"]["input_mask"]}
    nz = loop_noises(fx.loop_seed(TAG, "ddim50"), (B, L, E), 50, None)
    diff.noise_fn = lambda k, i, x: nz[k].to(DEV)
    tok = sampling.generate(m, diff, cond, step=50, noise=inp["gen_noise0"], sharded=False)
    assert tok.dtype == torch.int64 and tok.shape == (B, L)
    final = torch.from_numpy(np.asarray(load_golden("model_%s.npz" % TAG)["loop_ddim50"]))
    logits = odn.get_logits(sd, final, logits_mode=2)
    bound = torch.from_numpy(dr.scores(final.reshape(-1, E).numpy(), sd["lm_head.weight"].numpy())[1].max(1)).view(B, L)
    top2 = logits.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]).double() > bound
    assert int((~safe).sum()) <= 0.01 * safe.numel()
    assert torch.equal(tok.cpu()[safe], logits.argmax(-1)[safe])
    assert not torch.equal(tok.cpu(), odn.get_logits(sd, final).argmax(-1))        # mode 1's tokens are others


def test_unknown_logits_mode_raises():
    m, diff, c = build(3, train=True)
    with pytest.raises(NotImplementedError):
        m.argmax_tokens(torch.zeros(1, 2, c["E"], device=DEV))
    with pytest.raises(NotImplementedError):
        run_losses(m, diff, "plain")
    with pytest.raises(NotImplementedError):
        run_losses(m, diff, "corrupt")


def test_one_train_step_on_a_mode2_model():
    """TrainStep over a mode-2 model: lm_head.bias never receives a gradient and is skipped by the optimizer (bit-unchanged under weight
    decay, as torch.optim.AdamW leaves a parameter without a gradient), the tied table moves, and a position whose x_start sits exactly on
    its embedding row (its draw forced to 0: the clamp of the decoder NLL's target score) leaves every parameter finite"""
    m, diff, c = build(2, train=True)
    batch = fx.loss_inputs(TAG)["batch"]
    bias0, emb0 = m.lm_head.bias.detach().clone(), m.word_embedding.weight.detach().clone()
    loop = TrainStep(m, diff, lr=1e-3, weight_decay=0.01, ema_rate="0.9")

    class Draws(CpuDraws):
        def __enter__(self):
            super().__enter__()
            inner, self.calls = torch.randn_like, 0

            def fake(x, **kw):
                z = inner(x, **kw)
                if self.calls == 0:                      # the first draw is x_start's (diffusion.py:614)
                    z[0, 3, :] = 0.0
                self.calls += 1
                return z
            torch.randn_like = fake
            return self

    with Draws(5):
        losses, grad_norm = loop.run_step(batch)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()) and bool(torch.isfinite(grad_norm).all())
    assert m.lm_head.bias.grad is None and torch.equal(m.lm_head.bias.detach(), bias0)
    assert not torch.equal(m.word_embedding.weight.detach(), emb0)
    for n, p in m.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if n != "lm_head.bias":
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
