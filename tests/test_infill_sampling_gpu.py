"""GPU: sampling.infill / sampling.run_infill around the existing generate / modify paths, with the tiny random model of
tests/test_sampling_gpu.py (the "tiny" shape and seed with a position table of 128, so that a ComMU-shaped row fits).  What is pinned is
the mechanics - the plan, the same reverse loop as generate / modify under the plan's mask, the splice - not the music: the weights are
random.  With these weights the key token 610 does not come back from argmax_tokens (its embedding scores higher against token 18's
longer row), and the batch holds a piece in that key: the raw sampler output differs from the piece OUTSIDE the region, the spliced
output does not."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import infill_ref as ir  # noqa: E402
from musediffusion_amd import sampling  # noqa: E402
from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps  # noqa: E402
from musediffusion_amd.models.network import TransformerNetModel  # noqa: E402
from musediffusion_amd.utils import decode_util as du  # noqa: E402
from oracle import denoiser as odn  # noqa: E402
from oracle import fixtures as fx  # noqa: E402

DEV = "cuda"
L, E, STEP = 128, 32, 10
KINDS = ("clean", "extra_bar", "clean", "two_extra_bars", "clean", "no_eos")
BARS = [(1, 2), (0, 2), (2, 3), (1, 3), (0, 3), (0, 1)]               # per row; the last row has no EOS, whatever its range
NOT_PLANNED = 5


@pytest.fixture(scope="module")
def setup():
    c = dict(fx.CONFIGS["tiny"], L=L)
    sd = odn.random_state_dict(c["E"], c["H"], c["F"], c["nL"], c["V"], c["L"], c["Tt"], seed=fx.SEEDS["tiny"], emb_std=fx.EMB_STD)
    m = TransformerNetModel(c["E"], c["E"], c["Tt"], c["V"], c["L"], dropout=0.0, bert_hidden=c["H"], bert_layers=c["nL"], bert_heads=c["nh"],
                            bert_ffn=c["F"], compute_dtype="fp32")
    m.load_state_dict(sd)
    m.eval().requires_grad_(False).to(DEV)
    diff = SpacedDiffusion(use_timesteps=space_timesteps(2000, [2000]), betas=get_named_beta_schedule("sqrt", 2000), rescale_timesteps=True,
                           predict_xstart=True)
    g = np.random.default_rng(22)                                      # the seed whose first piece is in the key of token 610
    rows = [dr.make_row(g, L, k, n_bars=3, notes_per_bar=3) for k in KINDS]
    tokens, mask = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    assert tokens[0, 1] == 610
    cond = {"input_ids": torch.from_numpy(tokens).long(), "input_mask": torch.from_numpy(mask).long()}     # host tensors, as a loader hands them over
    gen = torch.Generator().manual_seed(5)
    noise = torch.randn(len(KINDS), L, E, generator=gen)
    steps = [torch.randn(len(KINDS), L, E, generator=gen) for _ in range(STEP)]
    return m, diff, cond, tokens, mask, noise, steps


def fixed_draws(diff, steps):
    diff.noise_fn = lambda k, i, x: steps[k].to(DEV)[:x.shape[0]]


def bars_tensor():
    return torch.tensor(BARS, dtype=torch.int32)


def test_infill_is_plan_generate_splice_bit_for_bit(setup):
    m, diff, cond, tokens, mask, noise, steps = setup
    fixed_draws(diff, steps)
    tok, res = sampling.infill(m, diff, cond, bars_tensor(), step=STEP, room=1, noise=noise, sharded=False)
    assert tok.dtype == torch.int64 and tok.shape == (len(KINDS), L) and tok.is_cuda
    plan = res.plan
    want = ir.plan_rows(tokens, mask, [b[0] for b in BARS], [b[1] for b in BARS], room=1)
    for k, t in (("tokens", plan.tokens), ("mask", plan.mask), ("status", plan.status), ("info", plan.info)):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    assert np.array_equal(plan.prefix_mask.cpu().numpy(), mask) and want["status"].tolist() == [0, 0, 0, 0, 0, ir.NO_EOS]
    plan_cond = {"input_ids": plan.tokens, "input_mask": plan.mask}
    raw = sampling.generate(m, diff, plan_cond, step=STEP, noise=noise, sharded=False)
    spliced, counts = du.splice_infill(plan, raw)
    assert torch.equal(tok, spliced.long()) and torch.equal(res.counts, counts) and res.status is plan.status
    # the splice matters: outside the region the raw argmax output is NOT the piece, the spliced output is
    raw, tok_h = raw.cpu().numpy(), tok.cpu().numpy()
    outside = want["mask"] == 0
    assert (raw[outside] != want["tokens"][outside]).any() and raw[0, 1] != 610
    for b in range(len(KINDS)):
        lo, hi, n_mask, added = want["info"][b]
        if b == NOT_PLANNED:
            assert np.array_equal(tok_h[b], tokens[b]), "a row that cannot be planned returns unchanged"
            continue
        kept = int(counts[b, 0])
        # [0, first region slot) is the piece; the kept notes follow; then the piece from the end of the region on, then pads
        assert np.array_equal(tok_h[b, :lo], tokens[b, :lo])
        rest = tokens[b, hi - added:L - added]
        n_bar = int((want["tokens"][b, lo:hi] == ir.BAR).sum())
        inner = tok_h[b, lo:lo + kept + n_bar]
        assert (inner == ir.BAR).sum() == n_bar and all(ir.token_class(t) >= 0 for t in inner[inner != ir.BAR])
        after = lo + kept + n_bar
        assert np.array_equal(tok_h[b, after:after + len(rest)], rest) and not tok_h[b, after + len(rest):].any()
    s = res.summary()
    assert s["rows"] == {"ok": 5, "no_eos": 1, "bad_mask": 0, "bad_range": 0, "overflow": 0}
    assert s["kept"] % 4 == 0 and s["kept"] + s["pads"] + s["other"] == int(want["info"][:, 2].sum()) and s["changed"] == 0


def test_infill_with_strength_is_plan_modify_splice_bit_for_bit(setup):
    m, diff, cond, tokens, mask, noise, steps = setup
    fixed_draws(diff, steps)
    tok, res = sampling.infill(m, diff, cond, (0, 1), step=STEP, strength=0.5, noise=noise, sharded=False)
    plan = res.plan
    raw = sampling.modify(m, diff, {"input_ids": plan.tokens, "input_mask": plan.mask}, step=STEP, strength=0.5, noise=noise, sharded=False)
    spliced, counts = du.splice_infill(plan, raw)
    assert torch.equal(tok, spliced.long()) and torch.equal(res.counts, counts)
    assert plan.status.tolist() == [0, 0, 0, 0, 0, ir.NO_EOS] and not plan.info[:, 3].any()
    outside = (plan.mask == 0).cpu().numpy()
    # room 0: nothing moves in front of the region, and a row that keeps all its region tokens is the piece outside it
    tok_h = tok.cpu().numpy()
    for b in range(len(KINDS)):
        lo = int(plan.info[b, 0])
        assert np.array_equal(tok_h[b, :lo], tokens[b, :lo]) or b == NOT_PLANNED
    assert np.array_equal(tok_h[NOT_PLANNED], tokens[NOT_PLANNED]) and outside[NOT_PLANNED].all()


def _bars_of(dec, b, notes):
    tpb = 480 * dr.BEATS[int(dec.meta[b, 2]) - 627]
    shift = 0 if int(dec.restored[b, 0]) == ir.BAR else 1
    return [int(n[0]) // tpb - shift for n in notes]


def test_decode_with_the_input_mask_keeps_the_other_bars(setup):
    m, diff, cond, tokens, mask, noise, steps = setup
    diff.noise_fn, diff.rng_mode = None, "philox"                      # the product's own draws
    checked = 0
    for room, fields in ((2, "all"), (0, "all"), (0, ("velocity", "duration"))):
        tok, res = sampling.infill(m, diff, cond, bars_tensor(), step=STEP, room=room, fields=fields)
        dev_mask = cond["input_mask"].to(DEV)
        orig = du.decode_tokens(cond["input_ids"].to(DEV), dev_mask, strict_validation=True)
        got = du.decode_tokens(tok, dev_mask, strict_validation=True)
        o_rows, g_rows = orig.cpu(), got.cpu()
        for b, (lo, hi) in enumerate(BARS):
            if o_rows.status[b] != du.OK:
                continue
            assert g_rows.status[b] in (du.OK, du.ONCE_FAILED), (room, fields, b, g_rows.status[b])
            if g_rows.status[b] == du.OK:
                keep = lambda rows, dec: [tuple(int(x) for x in n) for n, k in zip(rows.notes[b], _bars_of(dec, b, rows.notes[b])) if not lo <= k < hi]  # noqa: E731
                assert keep(g_rows, got) == keep(o_rows, orig), (room, fields, b)
                checked += 1
    assert checked >= 6


def test_fields_pitch_changes_only_pitch_slots(setup):
    m, diff, cond, tokens, mask, noise, steps = setup
    fixed_draws(diff, steps)
    tok, res = sampling.infill(m, diff, cond, bars_tensor(), step=STEP, fields="pitch", noise=noise, sharded=False)
    tok_h, counts = tok.cpu().numpy(), res.counts.cpu().numpy()
    assert res.plan.fields == 4 and np.array_equal(res.plan.tokens.cpu().numpy(), tokens)
    changed = tok_h != tokens
    pmask = res.plan.mask.cpu().numpy()
    assert (pmask[changed] == 1).all() and all(ir.token_class(t) == 2 for t in tokens[pmask == 1]) and all(ir.token_class(t) == 2 for t in tok_h[pmask == 1])
    assert np.array_equal(changed.sum(1), counts[:, 3]) and np.array_equal(counts[:, 0] + counts[:, 2], res.plan.info[:, 2].cpu().numpy())
    want = ir.plan_rows(tokens, mask, [b[0] for b in BARS], [b[1] for b in BARS], fields=4)
    assert not counts[NOT_PLANNED].any() and np.array_equal(pmask, want["mask"]) and pmask.sum(1).tolist() == [3, 3, 3, 3, 9, 0]
    with pytest.raises(ValueError):
        sampling.infill(m, diff, cond, (0, 1), step=STEP, fields="pitch", room=1)


def test_run_infill_with_and_without_an_output_directory(setup, tmp_path):
    m, diff, cond, tokens, mask, noise, steps = setup
    diff.noise_fn, diff.rng_mode = None, "philox"
    corrupted = cond["input_ids"].clone()
    corrupted[corrupted == ir.EOS] = 0                                 # what modification mode would start from: infill must not
    batch = {"input_ids": corrupted, "input_mask": cond["input_mask"], "correct_ids": cond["input_ids"]}
    loader = [batch, {k: v for k, v in batch.items() if k != "correct_ids"}]
    B = len(KINDS)
    logs = {}
    for where in (str(tmp_path / "out"), None):
        logs[where] = []
        rep = sampling.run_infill(m, diff, loader, bars=(0, 1), step=STEP, room=1, batch_size=B, out_dir=where, log=logs[where].append)
        assert rep.batches == 2 and isinstance(rep.total_valid_count, int)
        # first batch: planned on correct_ids (five rows, one without EOS); second: on input_ids, whose EOS the corruption removed
        assert rep.infill["rows"] == {"ok": 5, "no_eos": 1 + B, "bad_mask": 0, "bad_range": 0, "overflow": 0}
        assert rep.infill["kept"] % 4 == 0 and rep.infill["changed"] == 0 and any(ln.startswith("### Infill:") for ln in logs[where])
        assert rep.totals is not None and set(rep.summary) >= {"onnc", "cp", "cv"}
        if where:
            files = sorted(os.listdir(where))
            assert len(files) == rep.total_valid_count and all(f.endswith(".midi") and "_batch00000_" in f for f in files)
