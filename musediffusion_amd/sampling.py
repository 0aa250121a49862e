"""The reference's sampling run (run/sample.py:149-317).

`generate` / `modify` are its hot block (:185-220): everything between "a batch of token ids arrives" and "a batch of token ids
leaves", sharded over ranks when a process group is initialised.  `run_modification` / `run_generation` are the loop around it
(:168-317): per batch the sampler, ONE decode on the device (utils/decode_util.decode_tokens), the metrics of the batch from that same
decode (evaluation.evaluate_batch: 1NNC, CP, CV, the running totals - all device scalars) and, when an output directory is given, the
MIDI files through write_decoded_rows from one device -> host copy.  Without an output directory the modification loop does not sync
with the host before the final summary.  Generation mode has no ground truth; with get_metric it reports what needs none
(evaluation.evaluate_generated / GenerationTotals: diversity, duplicates, novelty against a corpus, CP, CV).  Not reproduced: tqdm /
logger / StringIO plumbing, reading training_args.json, and the rank-after-rank decode with its broadcasts (every rank holds the
gathered tokens of the global batch and computes the same totals; rank 0 writes the files).
Not in the reference: `infill` / `run_infill` regenerate a bar range, or single note fields inside it, and keep the rest of the piece -
a plan and a splice (utils/infill_util.py, csrc/infill.hip) around `generate` / `modify`, which run unchanged under the plan's mask.
Nor is `harmony=True` of the three loops: the batch's one decode also goes through evaluation.HarmonyTotals (csrc/harmony.hip) and
the report says how the notes fit the chords the pieces were conditioned on.  Nor is `constrained=True` of `generate` / `modify` and of the
loops: the final argmax becomes the best token sequence the decode path accepts (utils/grammar_util.py, csrc/grammar.hip), so that a
row is not lost to one token in the wrong place; the in-loop clamp (denoised_fn_round) stays as it is.  Nor is `region=` of `generate` /
`modify` and `rounding="region"` of `infill` / `run_infill`: the slots an infill plan masks are rounded to whole notes and pads
(gu.constrain_region_tokens, csrc/region.hip), so that the splice drops no token of a broken note.  Nor is `structure=True` of the
three loops: the batch's one decode also goes through evaluation.StructureTotals (csrc/structure.hip) and the report says how the
pieces are shaped over time - pitch-class entropy of 1-bar and 4-bar windows, groove similarity of the bars - next to the same
numbers of the ground truth (modification, infill) or of a summary the caller made from a training set (generation).  Nor are
`arrange` / `run_arrangement`: the batch is the tracks of several songs over one chord progression (utils/arrange_util.py), sampled
by `generate` as it is; the loop aligns the decoded tracks of a song, writes each complete song as ONE multitrack file and reports how
the tracks fit each other (evaluation.InterplayTotals, csrc/arrange.hip)."""
import contextlib
import io
import os
from functools import partial
from types import SimpleNamespace

import torch

from . import evaluation, metric, sharding
from .models.rounding import denoised_fn_round
from .utils import arrange_util as au, decode_util as du, grammar_util as gu


def _prepare(model, cond, device):
    ids = cond["input_ids"].to(device)
    mask = cond["input_mask"].to(device)
    x_start = model.get_embeds(ids)                                              # sample.py:185
    mask3 = torch.broadcast_to(mask.unsqueeze(dim=-1), x_start.shape)            # sample.py:186
    return x_start, mask3


def _solver(solver, solver_order):
    """-> the keyword arguments of _run that say which reverse loop runs ({} for the reference's)"""
    if solver not in ("ddim", "dpmpp"):
        raise ValueError("solver is 'ddim' or 'dpmpp', got %r" % (solver,))
    if solver == "ddim":
        return {}
    if solver_order not in (1, 2):
        raise ValueError("solver_order is 1 or 2, got %r" % (solver_order,))
    return {"solver": solver, "solver_order": solver_order}


def _run(model, diffusion, x_start, mask3, x_noised, step, noising_t, clip_denoised, top_p, clamp_step, constrain=None, solver="ddim",
         solver_order=2):
    T = diffusion.num_timesteps
    if solver == "dpmpp":
        # not in the reference: multistep DPM-Solver++ for every step count, the ancestral loop's (gap 1) included
        gap, sample_fn = max(1, T // step), partial(diffusion.dpmpp_sample_loop, order=solver_order)
    elif step == T:                                                               # sample.py:109-114
        gap, sample_fn = 1, diffusion.p_sample_loop
    else:
        gap, sample_fn = T // step, diffusion.ddim_sample_loop
    emb = torch.nn.Embedding(model.word_embedding.num_embeddings, model.word_embedding.embedding_dim,
                             _weight=model.word_embedding.weight.detach().clone()).eval().requires_grad_(False)
    samples = sample_fn(model=model, shape=tuple(x_start.shape), noise=x_noised, clip_denoised=clip_denoised,
                        denoised_fn=partial(denoised_fn_round, emb, dist=None), model_kwargs={}, top_p=top_p,
                        clamp_step=clamp_step, clamp_first=True, mask=mask3, x_start=x_start, gap=gap,
                        t_enc=noising_t, only_last=True)                          # sample.py:200-215
    if constrain is None:
        return model.argmax_tokens(samples[-1])                                   # sample.py:218-220
    return model.argmax_tokens(samples[-1], constrain=constrain)                  # -> (tokens, ConstrainResult | RegionResult)


def _constrain_args(local, bars, B, sharded):
    """argmax_tokens' `constrain` for this rank's rows: a per-row bars tensor [B, 2] of the GLOBAL batch is cut like the batch"""
    if isinstance(bars, torch.Tensor):
        lo, hi = sharding.shard_bounds(B) if sharded else (0, B)
        bars = bars[lo:hi]
    return local["input_ids"], local["input_mask"], bars


def _region_args(region, B, sharded):
    """argmax_tokens' `constrain` for this rank's rows: an infill plan of the GLOBAL batch is cut like the batch"""
    lo, hi = sharding.shard_bounds(B) if sharded else (0, B)
    return SimpleNamespace(tokens=region.tokens[lo:hi], mask=region.mask[lo:hi], status=region.status[lo:hi], fields=region.fields)


def _rounding(local, B, sharded, constrained, bars, region):
    """-> (argmax_tokens' `constrain` or None, the class of the result that comes back with the tokens or None)"""
    if region is not None:
        if constrained:
            raise ValueError("region= rounds the slots of an infill plan, constrained=True the whole note region of a row under a Bar "
                             "budget: one or the other")
        if tuple(region.tokens.shape) != (B,) + tuple(local["input_ids"].shape[1:]):
            raise ValueError("region: an infill plan of the GLOBAL batch, whose tokens / mask are cond's input_ids / input_mask")
        return _region_args(region, B, sharded), gu.RegionResult
    if constrained:
        return _constrain_args(local, bars, B, sharded), gu.ConstrainResult
    return None, None


def _gather(out, B, sharded, result):
    """the local shard's tokens - with a `result` class (tokens, ConstrainResult | RegionResult), every tensor of it - gathered to the
    global batch"""
    if result is None:
        return sharding.gather_rows(out, B) if sharded else out
    tokens, res = out
    if sharded:
        tokens = sharding.gather_rows(tokens, B)
        res = result(*(sharding.gather_rows(t, B) for t in (res.status, res.path_score, res.counts)))
    return tokens, res


@torch.no_grad()
def generate(model, diffusion, cond, step=None, clip_denoised=True, top_p=1, clamp_step=0, sharded=True, noise=None,
             t_enc=None, constrained=False, bars="exact", region=None, solver="ddim", solver_order=2):
    """Generation mode: noise everywhere except the anchored meta prefix (run/sample.py:190-193).
    `cond` = {'input_ids', 'input_mask'} for the GLOBAL batch; returns int64 tokens [B, L] on every rank.
    Additions to the reference's block: `noise` = the start latent's draw for the GLOBAL batch (each rank takes its rows;
    default: this rank's `torch.randn_like`, as the reference), `t_enc` = stop after that many iterations
    (the loops' own argument, diffusion.py:425); `constrained` = round the last latent to the best row the decode path accepts
    (grammar_util.constrain_tokens with `bars`, on the local shard before the gather) and return (tokens, ConstrainResult), both for
    the GLOBAL batch; `region` = an infill plan (du.plan_infill) of the GLOBAL batch whose tokens / mask are `cond`'s input_ids /
    input_mask: round the plan's masked slots to whole notes (grammar_util.constrain_region_tokens on the local shard, the plan cut to
    this rank's rows like the batch) and return (tokens, RegionResult) for the GLOBAL batch.  `region` together with constrained=True
    raises ValueError.  `solver`: "ddim" - the reference's loops, ancestral at step == T and its DDIM otherwise - or "dpmpp": the
    multistep DPM-Solver++ loop (diffusion.dpmpp_sample_loop, gap = T // step) of order `solver_order` (1 or 2); the roundings after
    the loop (`constrained`, `region`) are the same."""
    how = _solver(solver, solver_order)
    device = model.word_embedding.weight.device
    B = cond["input_ids"].shape[0]
    local = sharding.shard_batch(cond) if sharded else cond
    constrain, result = _rounding(local, B, sharded, constrained, bars, region)
    x_start, mask3 = _prepare(model, local, device)
    if noise is None:
        noise = torch.randn_like(x_start)
    else:
        lo, hi = sharding.shard_bounds(B) if sharded else (0, B)
        noise = noise[lo:hi].to(device)
    x_noised = torch.where(torch.eq(mask3, 0), x_start, noise)
    out = _run(model, diffusion, x_start, mask3, x_noised, step or diffusion.num_timesteps, t_enc, clip_denoised,
               top_p, clamp_step, constrain, **how)
    return _gather(out, B, sharded, result)


@torch.no_grad()
def modify(model, diffusion, cond, step, strength=0.75, clip_denoised=True, top_p=1, clamp_step=0, sharded=True, noise=None,
           constrained=False, bars="exact", region=None, solver="ddim", solver_order=2):
    """Modification mode: q_sample the corrupted sequence to noising_t = int(step * strength), then
    run the reverse loop for noising_t iterations (run/sample.py:195-197, :214).  `noise`: q_sample's draw for the
    GLOBAL batch, [B, L, E] (default: this rank's device generator, as the reference).  `constrained`, `bars`, `region`: as in
    `generate`; so are `solver` and `solver_order`."""
    how = _solver(solver, solver_order)
    device = model.word_embedding.weight.device
    B = cond["input_ids"].shape[0]
    local = sharding.shard_batch(cond) if sharded else cond
    constrain, result = _rounding(local, B, sharded, constrained, bars, region)
    x_start, mask3 = _prepare(model, local, device)
    noising_t = int(step * strength)
    timestep = torch.full((x_start.shape[0], 1), noising_t - 1, device=device)
    if noise is not None:
        lo, hi = sharding.shard_bounds(B) if sharded else (0, B)
        noise = noise[lo:hi].to(device).unsqueeze(-1)
    x_noised = diffusion.q_sample(x_start.unsqueeze(-1), timestep, noise=noise, mask=mask3).squeeze(-1)
    out = _run(model, diffusion, x_start, mask3, x_noised, step, noising_t, clip_denoised, top_p, clamp_step, constrain, **how)
    return _gather(out, B, sharded, result)


@torch.no_grad()
def infill(model, diffusion, cond, bars, step=None, strength=1.0, room=0, fields="all", clip_denoised=True, top_p=1, clamp_step=0,
           sharded=True, noise=None, constrained=False, rounding="argmax", solver="ddim", solver_order=2):
    """Not in the reference: keep the piece, regenerate bars lo <= k < hi (`bars` = (lo, hi) or an int tensor [B, 2]) - all of their
    notes, with `room` more note slots per bar, or with `fields` ('pitch', ('velocity', 'duration'), ...) only those tokens of their
    notes.  du.plan_infill makes the row and the mask on the GLOBAL batch; the existing paths run under that mask - strength == 1:
    `generate` (noise in the region, all steps), else `modify` (q_sample to int(step * strength)); du.splice_infill brings the gathered
    tokens back: the original tokens outside the region bit for bit, whole notes inside it.  -> (tokens [B, L] int64, du.InfillResult).
    Decode the tokens with cond['input_mask'], not with the plan's mask.  A row that cannot be planned returns unchanged and says why
    in the result's status.  rounding: 'argmax' (every region slot by its own argmax; the splice drops every pad, every token of a
    broken note and every field slot of the wrong class) or 'region' (the same `generate` / `modify` call with region=plan: the region
    leaves the sampler as whole notes and pads, or per field slot the best token of that field, so the splice drops pads only; the
    result's `.rounding` is the gu.RegionResult, None for 'argmax').  constrained=True is refused: the plan's region sits in the middle
    of the row between tokens that must stay, which the row grammar with its Bar budget does not express; rounding='region' is the
    rounding for an infill.  solver, solver_order: `generate`'s."""
    if constrained:
        raise NotImplementedError("infill(constrained=True): the regenerated region lies mid-row between kept tokens; grammar-constrained "
                                  "rounding needs fixed-token positions for that and covers generate / modify only")
    if rounding not in ("argmax", "region"):
        raise ValueError("infill: rounding is 'argmax' or 'region', got %r" % (rounding,))
    loop = _solver(solver, solver_order)
    device = model.word_embedding.weight.device
    plan = du.plan_infill(cond["input_ids"].to(device), cond["input_mask"].to(device), bars, room, fields)
    plan_cond = {"input_ids": plan.tokens, "input_mask": plan.mask}
    how = {"region": plan} if rounding == "region" else {}
    if strength == 1:
        raw = generate(model, diffusion, plan_cond, step, clip_denoised, top_p, clamp_step, sharded=sharded, noise=noise, **how, **loop)
    else:
        raw = modify(model, diffusion, plan_cond, step or diffusion.num_timesteps, strength, clip_denoised, top_p, clamp_step,
                     sharded=sharded, noise=noise, **how, **loop)
    raw, rounded = raw if how else (raw, None)
    tokens, counts = du.splice_infill(plan, raw)
    return tokens.to(torch.int64), du.InfillResult(plan, counts, rounded)


# ------------------------------------------------------------------------------------------------ the loop around the hot block
class SamplingReport:
    """What a run leaves: total_valid_count (int), totals (evaluation.MetricTotals - a generation run with get_metric:
    evaluation.GenerationTotals - or None), summary (the totals' summary() dict or None), batches (how many the loop ran).  A run with
    harmony=True adds `harmony` (evaluation.HarmonyTotals.summary(), or None when no batch ran); run_infill adds `infill` and, with
    rounding='region', `region` (gu.RegionResult.describe over all batches: rows per status, masked slots, notes, pads, segments); a run with
    constrained=True adds `constrained` (gu.ConstrainResult.describe over all batches: rows per status, Bars and notes placed); a run with
    structure=True adds `structure` ({"generated"[, "reference", "gap"]}: evaluation.StructureTotals summaries and their
    evaluation.structure_gap, or None when no batch ran); run_arrangement adds `songs` (the songs written, or that would have been
    without an output directory) and `interplay` (evaluation.InterplayTotals.summary(), or None with interplay=False or when no
    batch ran) and `choice` (candidates > 1: the sums of the chosen and the unchosen fit, else None) - its total_valid_count counts
    the tracks that decoded."""

    def __init__(self, total_valid_count, totals, summary, batches):
        self.total_valid_count, self.totals, self.summary, self.batches = total_valid_count, totals, summary, batches


def _write_rows(mode, rows, batch_index, previous_count, out_dir, log):
    """write_decoded_rows with its report going to `log` (the reference: redirect_stdout into the log file and stdout)"""
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            return du.write_decoded_rows(mode, rows, batch_index, previous_count, out_dir, return_indices=True)
    finally:
        if out.getvalue():
            log(out.getvalue())


def _constrained_block(d):
    """the log block of a run with constrained=True"""
    rows = d["rows"]
    total = sum(rows.values())
    kept = ", ".join("%s %d" % (k, v) for k, v in rows.items() if k != "ok" and v)
    return ("### Grammar-constrained rounding: %d of %d rows rounded to an accepted sequence (%d Bars, %d notes)%s" % (
        rows["ok"], total, d["bars"], d["notes"], "; left as the plain argmax: " + kept if kept else ""))


def _choice_block(c, candidates):
    """the log block of run_arrangement with candidates > 1"""
    return ("### Tracks chosen among %d candidates: %d songs, %d with another choice than candidate 0 everywhere\n"
            "    Fit of the chosen tracks: %d (without choosing: %d)" % (candidates, c["songs"], c["changed"], c["best"], c["first"]))


def _structure_report(generated, reference, given, log):
    """a loop's `structure`: the summaries of its StructureTotals (`reference`: the ground truth's, or None) from ONE device -> host
    copy, or `given` (a summary made beforehand) as the reference; logged as evaluation.structure_block"""
    n = len(evaluation.StructureTotals.INT_NAMES) + len(evaluation.StructureTotals.FLOAT_NAMES)
    host = torch.cat([generated.vector()] + ([reference.vector()] if reference is not None else [])).cpu().tolist()
    ref = evaluation.StructureTotals.ratios(host[n:]) if reference is not None else given
    out = evaluation.structure_report(evaluation.StructureTotals.ratios(host[:n]), ref)
    log(evaluation.structure_block(out["generated"]))
    if ref is not None:
        log(evaluation.structure_block(out["reference"], "Structure of the reference"))
        log(evaluation.structure_block(out["gap"], "Structure gap"))
    return out


def _fatal_status(rows):
    """the first status of a DecodedRows on which write_decoded_rows raises, or 0"""
    for st in rows.status:
        if int(st) != du.OK and int(st) not in evaluation._INVALID:
            return int(st)
    return 0


@torch.no_grad()
def run_modification(model, diffusion, data_loader, *, step, strength=0.75, batch_size, out_dir=None, get_metric=True, sampler=None,
                     clip_denoised=True, top_p=1, clamp_step=0, log=print, harmony=False, harmony_bars=None, constrained=False,
                     bars="exact", solver="ddim", solver_order=2, structure=False):
    """run/sample.py:168-317 in modification mode.  data_loader yields {'input_ids', 'input_mask'[, 'correct_ids']} for the GLOBAL
    batch; `sampler(cond)` returns its tokens [B, L] (default: `modify`, sharded when a process group is up).  With get_metric and a
    'correct_ids' in the batch: evaluation.evaluate_batch (strict validation, as the reference when it computes metrics) and the
    running totals.  With out_dir: rank 0 writes one file per valid row, named as decode_batch names them (previous_count =
    batch_index * batch_size), from the same decode - one decode and one device -> host copy per batch - and the metric block of the
    batch is logged right after it.  Without out_dir nothing is read back until the loop ends: the blocks of all batches are logged
    then, before the summary, from ONE copy.  Returns a SamplingReport.
    harmony (an addition): the DecodedBatch every batch has anyway also goes through evaluation.HarmonyTotals - one more launch per
    batch, one more device -> host copy after the loop - and the report gains `harmony`, its summary (CH: do the notes fit the chords
    the piece was conditioned on), logged as evaluation.harmony_block; harmony_bars: HarmonyTotals.update's `bars`.
    constrained (an addition): the sampler rounds to the best row the decode path accepts (`modify(constrained=True, bars=bars)`; a
    `sampler` of the caller's then returns (tokens, ConstrainResult) too).  Two more launches per batch, one more device -> host copy
    after the loop; the report gains `constrained` and _constrained_block is logged.  Without it nothing changes.
    solver, solver_order (an addition): `modify`'s - which reverse loop the default sampler runs.
    structure (an addition): the batch's DecodedBatch also goes through evaluation.StructureTotals - one more launch per batch - and,
    when the batch has 'correct_ids', the ground truth is decoded too (one more decode per batch, validated as the sample is) into a
    second StructureTotals; one more device -> host copy after the loop for both.  The report gains `structure` = {"generated",
    "reference", "gap"} (without ground truth: "generated" only), logged as evaluation.structure_block.  Without it nothing changes."""
    loop = _solver(solver, solver_order)
    if sampler is None:
        sampler = lambda cond: modify(model, diffusion, cond, step, strength, clip_denoised, top_p, clamp_step, sharded=True,  # noqa: E731
                                      **({"constrained": True, "bars": bars} if constrained else {}), **loop)
    write = out_dir is not None and sharding.rank() == 0
    if write:
        os.makedirs(out_dir, exist_ok=True)
    totals, total_valid, pending, batches = None, None, [], 0
    chord_fit, rounded, shape, shape_ref = None, None, None, None
    for batch_index, cond in enumerate(data_loader):
        tokens = sampler(cond)
        if constrained:
            tokens, res = tokens
            rounded = res.vector() if rounded is None else rounded + res.vector()
        dev = tokens.device
        mask = cond["input_mask"].to(dev)
        metric_on = bool(get_metric) and cond.get("correct_ids") is not None
        if metric_on:
            if totals is None:
                log("### with calculating metrics ...")
                totals = evaluation.MetricTotals(dev)
            m = evaluation.evaluate_batch(tokens, cond["correct_ids"].to(dev), mask, strict_validation=True)
            totals.update(m)
            dec, count = m.decoded, m.valid_count
        else:
            dec = du.decode_tokens(tokens, mask, strict_validation=False)
            count = (dec.status == du.OK).sum()
        total_valid = count.clone() if total_valid is None else total_valid + count
        if harmony:
            chord_fit = (chord_fit or evaluation.HarmonyTotals(dev)).update(dec, bars=harmony_bars)
        if structure:
            shape = (shape or evaluation.StructureTotals(dev)).update(dec)
            if cond.get("correct_ids") is not None:
                truth = du.decode_tokens(cond["correct_ids"].to(dev), mask, strict_validation=metric_on)
                shape_ref = (shape_ref or evaluation.StructureTotals(dev)).update(truth)
        if out_dir is not None:
            rows = dec.cpu()
            if write:
                _write_rows("modification", rows, batch_index, batch_index * batch_size, out_dir, log)
            else:
                evaluation.MetricTotals.raise_if_fatal(_fatal_status(rows))
            if metric_on:
                host = m.vector().cpu().tolist()
                if host[0]:
                    log(evaluation.batch_block(batch_index, *host[1:]))
        elif metric_on:
            pending.append((batch_index, m.vector()))
        batches += 1
    if total_valid is None:
        report = SamplingReport(0, None, None, 0)
        if harmony:
            report.harmony = None
        if constrained:
            report.constrained = None
        if structure:
            report.structure = None
        return report
    # the one copy of a run without out_dir: [total valid | the seven of MetricTotals.vector() | six per pending batch]
    parts = [total_valid.double().reshape(1), totals.vector() if totals is not None else torch.zeros(7, device=total_valid.device, dtype=torch.float64)]
    host = torch.cat(parts + [v for _, v in pending]).cpu().tolist()
    for n, (batch_index, _) in enumerate(pending):
        rec = host[8 + 6 * n:14 + 6 * n]
        if rec[0]:
            log(evaluation.batch_block(batch_index, *rec[1:]))
    summary = None
    if totals is not None:
        evaluation.MetricTotals.raise_if_fatal(host[7])
        summary = evaluation.MetricTotals.ratios(host[1:7])
        log(evaluation.summary_block(summary))
    if out_dir is not None:
        log(f"### Written the decoded output to {out_dir}")
    report = SamplingReport(int(host[0]), totals, summary, batches)
    if harmony:
        report.harmony = chord_fit.summary()
        log(evaluation.harmony_block(report.harmony))
    if constrained:
        report.constrained = gu.ConstrainResult.describe(rounded.cpu().tolist())
        log(_constrained_block(report.constrained))
    if structure:
        report.structure = _structure_report(shape, shape_ref, None, log)
    return report


@torch.no_grad()
def run_infill(model, diffusion, data_loader, *, bars, step, strength=1.0, room=0, fields="all", batch_size, out_dir=None, get_metric=True,
               clip_denoised=True, top_p=1, clamp_step=0, log=print, harmony=False, rounding="argmax", solver="ddim", solver_order=2,
               structure=False):
    """run_modification with `infill` as its sampler: every batch is sampled on its 'correct_ids' where present (the piece itself; its
    'input_ids' are the corrupted copy modification mode starts from), else on 'input_ids', and decoded with the batch's own
    'input_mask'.  Files, numbering, metric blocks and the SamplingReport are that loop's; the report also carries `infill`: the
    InfillResult counts summed over the run (rows per status, kept / pads / other / changed), from one more device -> host copy at
    the end.  harmony: run_modification's, with this run's `bars`: the report's `harmony` also says how the regenerated bars
    (ch_region) and the kept ones (ch_rest) fit their chords.  rounding: `infill`'s; with 'region' the report gains `region`, the
    RegionResult counts summed over the run (rows per status, masked slots, notes and pads placed, segments) from one more device ->
    host copy after the loop, and one more line is logged.  Without it nothing changes: the same launches, copies and log.
    solver, solver_order: `infill`'s.  structure: run_modification's - with 'correct_ids' the reference is the piece itself."""
    if rounding not in ("argmax", "region"):
        raise ValueError("run_infill: rounding is 'argmax' or 'region', got %r" % (rounding,))
    how = {"rounding": rounding} if rounding != "argmax" else {}
    how.update(_solver(solver, solver_order))
    acc, racc = [], []

    def sampler(cond):
        ids = cond["correct_ids"] if cond.get("correct_ids") is not None else cond["input_ids"]
        tokens, res = infill(model, diffusion, {"input_ids": ids, "input_mask": cond["input_mask"]}, bars, step, strength, room, fields,
                             clip_denoised, top_p, clamp_step, sharded=True, **how)
        acc[:] = [res.vector() if not acc else acc[0] + res.vector()]
        if res.rounding is not None:
            racc[:] = [res.rounding.vector() if not racc else racc[0] + res.rounding.vector()]
        return tokens

    report = run_modification(model, diffusion, data_loader, step=step, strength=strength, batch_size=batch_size, out_dir=out_dir,
                              get_metric=get_metric, sampler=sampler, log=log, harmony=harmony, harmony_bars=bars if harmony else None,
                              **({"structure": True} if structure else {}))
    report.infill = du.InfillResult.describe(acc[0].cpu().tolist() if acc else [0] * 9)
    log("### Infill: rows %s, region tokens kept %d, pads dropped %d, other dropped %d, changed %d" % (
        report.infill["rows"], report.infill["kept"], report.infill["pads"], report.infill["other"], report.infill["changed"]))
    if how:
        report.region = gu.RegionResult.describe(racc[0].cpu().tolist() if racc else [0] * 9)
        log("### Region rounding: rows %s, notes placed %d, pads placed %d" % (
            report.region["rows"], report.region["notes"], report.region["pads"]))
    return report


@torch.no_grad()
def run_generation(model, diffusion, midi_meta_dict, *, batch_size, seq_len, num_samples, step=None, out_dir, sampler=None,
                   max_batches=None, clip_denoised=True, top_p=1, clamp_step=0, log=print, device="cuda", get_metric=False, corpus=None,
                   duplicate_threshold=None, harmony=False, constrained=False, bars="exact", solver="ddim", solver_order=2,
                   structure=False, structure_reference=None):
    """run/sample.py:168-317 in generation mode: ONE meta_to_batch, sampled again and again (infinite_loader_from_single); every batch
    is decoded without strict validation and its valid rows are written as generated_{n:0>7}.midi, n counting on from the running
    total_valid_count (out_dir None: decoded and counted, nothing written).  The loop stops after the batch that reaches num_samples
    - like the reference it may write more than num_samples files.  max_batches is an addition: the reference loops forever when no
    row is ever valid.  `sampler(cond)` defaults to `generate`, sharded when a process group is up.  Returns a SamplingReport.
    get_metric (an addition: the reference reports nothing about a generated set, having no ground truth): every batch goes through
    evaluation.evaluate_generated instead of the plain decode - the same decode, from which the files are written as before - and
    evaluation.GenerationTotals keeps its vectors; after the loop the summary (diversity, duplicates, CP, CV and, with `corpus` =
    [n, 56] get_vectors rows of a training set, novelty and memorised) is logged and fills the report's totals / summary.
    duplicate_threshold: GenerationTotals' (None: its default).  harmony: as in run_modification - the batch's one decode also goes
    through evaluation.HarmonyTotals and the report gains `harmony`.  constrained, bars: as in run_modification, with
    `generate(constrained=True, bars=bars)` - the report gains `constrained`, from one more copy after the loop.
    solver, solver_order: `generate`'s - which reverse loop the default sampler runs.
    structure: as in run_modification - the batch's one decode also goes through evaluation.StructureTotals (one more launch per
    batch, one more copy after the loop) and the report gains `structure` = {"generated"}; structure_reference: a
    StructureTotals.summary() dict made beforehand from a training set - the report then also carries it as "reference" and the
    "gap" to it."""
    loop = _solver(solver, solver_order)
    if sampler is None:
        sampler = lambda cond: generate(model, diffusion, cond, step, clip_denoised, top_p, clamp_step, sharded=True,  # noqa: E731
                                        **({"constrained": True, "bars": bars} if constrained else {}), **loop)
    cond = du.meta_to_batch(midi_meta_dict, batch_size, seq_len, device)
    write = out_dir is not None and sharding.rank() == 0
    if write:
        os.makedirs(out_dir, exist_ok=True)
    total, batch_index, totals, chord_fit, rounded, shape = 0, 0, None, None, None, None
    while total < num_samples and (max_batches is None or batch_index < max_batches):
        tokens = sampler(cond)
        if constrained:
            tokens, res = tokens
            rounded = res.vector() if rounded is None else rounded + res.vector()
        mask = cond["input_mask"].to(tokens.device)
        if get_metric:
            if totals is None:
                log("### with calculating metrics ...")
                kw = {} if duplicate_threshold is None else {"duplicate_threshold": duplicate_threshold}
                totals = evaluation.GenerationTotals(tokens.device, corpus=corpus, **kw)
            m = evaluation.evaluate_generated(tokens, mask, strict_validation=False)
            totals.update(m)
            dec = m.decoded
        else:
            dec = du.decode_tokens(tokens, mask, strict_validation=False)
        if harmony:
            chord_fit = (chord_fit or evaluation.HarmonyTotals(tokens.device)).update(dec)
        if structure:
            shape = (shape or evaluation.StructureTotals(tokens.device)).update(dec)
        rows = dec.cpu()
        if write:
            valid_count, _ = _write_rows("generation", rows, batch_index, total, out_dir, log)
        else:
            evaluation.MetricTotals.raise_if_fatal(_fatal_status(rows))
            valid_count = sum(1 for st in rows.status if int(st) == du.OK)
        total += valid_count
        batch_index += 1
    summary = None
    if totals is not None:
        summary = totals.summary()                            # the one copy of the metrics: pair statistics over every kept row
        log(evaluation.generation_block(summary))
    if out_dir is not None:
        log(f"### Written the decoded output to {out_dir}")
    report = SamplingReport(total, totals, summary, batch_index)
    if harmony:
        report.harmony = chord_fit.summary() if chord_fit is not None else None
        if chord_fit is not None:
            log(evaluation.harmony_block(report.harmony))
    if constrained:
        report.constrained = gu.ConstrainResult.describe(rounded.cpu().tolist()) if rounded is not None else None
        if rounded is not None:
            log(_constrained_block(report.constrained))
    if structure:
        report.structure = _structure_report(shape, None, structure_reference, log) if shape is not None else None
    return report


# ------------------------------------------------------------------------------------------------ from single tracks to songs
def choose_candidates(decoded, S, T, K, weights=None, unary=None):
    """decoded: the DecodedBatch of a candidate batch (au.candidate_batch: S songs x T tracks x K candidates) -> metric.TrackChoice
    with `rows` int64 [S * T]: the chosen row of every track of every song.  au.anchor_shift, then two library launches -
    metric.pair_fit (rows that did not decode and drum rows masked, as evaluation.InterplayTotals masks them: a drum note number is
    no pitch) and metric.choose_tracks on metric.fit_scores(., weights) with `unary` [S, T * K] int64 or None - and torch operations;
    nothing syncs with the host.  Eligible is every row that decoded OK, drum rows included: their pair scores are zero.  A track
    without an eligible candidate keeps candidate 0, whose decode status says that it failed."""
    ok = decoded.status == du.OK
    fit = metric.pair_fit(decoded, S, T, K, shift=au.anchor_shift(decoded), valid=ok & (decoded.meta[:, 5] != metric.DRUMS_INST))
    res = metric.choose_tracks(metric.fit_scores(fit.ticks, weights), S, T, K, unary=unary, eligible=ok.view(S, T * K))
    res.rows = (torch.arange(S * T, device=ok.device, dtype=torch.int64) * K + res.choice.clamp(min=0).view(-1).long())
    return res


@torch.no_grad()
def arrange(model, diffusion, base_meta, tracks, n_songs, seq_len, candidates=1, weights=None, unary=None, **generate_keywords):
    """`generate` on au.arrangement_batch(base_meta, tracks, n_songs, seq_len), nothing else: every row is one track of one song,
    the rows of a song share the chord progression, tempo, key and time signature of `base_meta` and differ in what `tracks`
    overrides (inst, track_role, pitch_range, min_velocity, max_velocity).  generate_keywords: `generate`'s (step, noise, solver,
    constrained, ...).  -> (generate's result, song [B], track [B], cond).
    candidates = K > 1: `generate` on au.candidate_batch (every track K times; `noise` is the candidate batch's), ONE decode, and
    choose_candidates(., weights, unary) keeps of every track the candidate of the best-fitting combination -> (the chosen tokens
    [n_songs * T, L], song, track and cond of the chosen rows, the metric.TrackChoice with choice, best, first, status and rows).
    A generate result with a second part (constrained, region) is not carried through the choice: ValueError."""
    device = model.word_embedding.weight.device
    if int(candidates) == 1:
        cond, song, track = au.arrangement_batch(base_meta, tracks, n_songs, seq_len, device)
        return generate(model, diffusion, cond, **generate_keywords), song, track, cond
    if generate_keywords.get("constrained") or generate_keywords.get("region") is not None:
        raise ValueError("arrange: candidates > 1 returns the chosen tokens only (no constrained / region result)")
    T, K = len(tracks), int(candidates)
    cond, song, track, _ = au.candidate_batch(base_meta, tracks, n_songs, seq_len, K, device)
    tokens = generate(model, diffusion, cond, **generate_keywords)
    dec = du.decode_tokens(tokens, cond["input_mask"].to(tokens.device), strict_validation=False)
    res = choose_candidates(dec, n_songs, T, K, weights, unary)
    rows = res.rows
    return (tokens.index_select(0, rows), song.index_select(0, rows.to(song.device)), track.index_select(0, rows.to(track.device)),
            {k: v.index_select(0, rows.to(v.device)) for k, v in cond.items()}, res)


@torch.no_grad()
def run_arrangement(model, diffusion, base_meta, tracks, *, n_songs, seq_len, num_songs, out_dir, step=None, keep_partial=False,
                    interplay=True, max_batches=None, sampler=None, clip_denoised=True, top_p=1, clamp_step=0, log=print, device="cuda",
                    solver="ddim", solver_order=2, candidates=1, weights=None):
    """run_generation for songs: ONE au.arrangement_batch of n_songs songs (len(tracks) rows each), sampled again and again until
    num_songs songs are complete (or max_batches batches ran).  Per batch the sampler (`sampler(cond)`, default `generate`, sharded
    when a process group is up), ONE decode without strict validation, au.align_shift (torch operations) and, with `interplay`, one
    more library launch (evaluation.InterplayTotals.update with the shifts; drum rows masked).  A song is complete iff every one of
    its tracks decoded OK; complete songs are written by au.write_song as song_{n:0>7}.midi, n counting on over the run, with the
    chord markers of the song's first track (out_dir None: decoded and counted, nothing written).  keep_partial: songs with at least
    two decoded tracks are written too, from the tracks that decoded, and count.  Rows of a fatal status raise as in run_generation.
    Returns a SamplingReport: total_valid_count = the tracks that decoded, batches, `songs` = the songs that count and `interplay` =
    the summary from one more device -> host copy after the loop, logged as evaluation.interplay_block (None without `interplay` or
    when no batch ran).
    candidates = K > 1: the batch is au.candidate_batch (every track K times), decoded once; choose_candidates (two more library
    launches per batch) keeps one candidate a track and one gather leaves the decoded batch of the chosen rows, on which everything
    above runs unchanged.  The report gains `choice`: {"best", "first"}: the sums of the chosen and of the unchosen objective over the
    songs of status OK or PARTIAL, "songs": their number, "changed": those whose choice is not candidate 0 everywhere - from one more
    device -> host copy after the loop, logged as one block; None at candidates = 1 or when no batch ran."""
    loop = _solver(solver, solver_order)
    if sampler is None:
        sampler = lambda cond: generate(model, diffusion, cond, step, clip_denoised, top_p, clamp_step, sharded=True, **loop)  # noqa: E731
    T, K = len(tracks), int(candidates)
    if K == 1:
        cond, song, _ = au.arrangement_batch(base_meta, tracks, n_songs, seq_len, device)
    else:
        cond, _, _, _ = au.candidate_batch(base_meta, tracks, n_songs, seq_len, K, device)
        song = torch.arange(n_songs, device=device, dtype=torch.int32).repeat_interleave(T)
    chosen = None                                                         # int64 [4] on the device: best, first, songs, changed
    write = out_dir is not None and sharding.rank() == 0
    if write:
        os.makedirs(out_dir, exist_ok=True)
    songs, valid_rows, batch_index, fit = 0, 0, 0, None
    while songs < num_songs and (max_batches is None or batch_index < max_batches):
        tokens = sampler(cond)
        dec = du.decode_tokens(tokens, cond["input_mask"].to(tokens.device), strict_validation=False)
        if K > 1:
            res = choose_candidates(dec, n_songs, T, K, weights)
            dec = dec.select(res.rows)
            counted = (res.status == metric.CHOOSE_OK) | (res.status == metric.CHOOSE_PARTIAL)
            moved = counted & (res.choice > 0).any(1)
            zero = torch.zeros_like(res.best)
            now = torch.stack([torch.where(counted, res.best, zero).sum(), torch.where(counted, res.first, zero).sum(),
                               counted.sum(), moved.sum()])
            chosen = now if chosen is None else chosen + now
        shift = au.align_shift(dec, song.to(tokens.device))
        if interplay:
            fit = (fit or evaluation.InterplayTotals(tokens.device)).update(dec, song, shift=shift)
        rows, shifts = dec.cpu(), shift.cpu().tolist()
        evaluation.MetricTotals.raise_if_fatal(_fatal_status(rows))
        for s in range(n_songs):
            ok = [b for b in range(s * T, (s + 1) * T) if int(rows.status[b]) == du.OK]
            valid_rows += len(ok)
            if len(ok) < (min(2, T) if keep_partial else T):
                continue
            if write:
                au.write_song(os.path.join(out_dir, f"song_{songs:0>7}.midi"), [rows.notes[b] for b in ok], rows.chords[ok[0]] + [shifts[ok[0]], 0],
                              rows.meta[ok], [shifts[b] for b in ok], [au.track_name(rows.meta[b], b - s * T) for b in ok])
            songs += 1
        log(f"### Batch {batch_index}: {songs} songs so far")
        batch_index += 1
    if out_dir is not None:
        log(f"### Written the decoded output to {out_dir}")
    report = SamplingReport(valid_rows, None, None, batch_index)
    report.songs = songs
    report.interplay = fit.summary() if fit is not None else None
    if fit is not None:
        log(evaluation.interplay_block(report.interplay))
    report.choice = None
    if chosen is not None:
        report.choice = dict(zip(("best", "first", "songs", "changed"), chosen.cpu().tolist()))
        log(_choice_block(report.choice, K))
    return report
