"""Grammar-constrained rounding (include/musehip_grammar.h, csrc/grammar.hip): the last act of a sampling run, made to leave rows the
decode path accepts.  Not in the reference, whose run/sample.py:218-220 takes the argmax of every position on its own and whose
decode_util.py then drops every row with one token in the wrong place.

`constrain_tokens` is two launches: ops.class_argmax (the argmax kernel's scores reduced per token class) and `constrain_rows` (one
wave per row: a Viterbi pass over the note region and its trace-back).  A row that cannot be constrained leaves exactly as
model.argmax_tokens leaves it and says why in the result's status.  Nothing here syncs with the host.

`constrain_region_tokens` is the same for an infill (include/musehip_region.h, csrc/region.hip): the class tables, then
`constrain_regions` - one block per row, one thread per maximal run of the plan's mask, ( PAD | POSITION VELOCITY PITCH DURATION )* in
each - so that utils/infill_util.splice_infill finds whole notes in the region and drops nothing but the pads."""
import torch

from .. import ops
from .._lib import ABI, check, current_stream, lib, ptr, require_device

# mirror of enum mhg_status / enum mhg_bars (include/musehip_grammar.h)
_GRAMMAR = ABI["musehip_grammar.h"].enums
(CONSTRAIN_OK, CONSTRAIN_BAD_MASK, CONSTRAIN_NO_CHORDS, CONSTRAIN_TOO_MANY_BARS, CONSTRAIN_BAD_BOUNDS, CONSTRAIN_NO_ROOM,
 CONSTRAIN_NONFINITE) = (_GRAMMAR["MHG_" + n] for n in ("OK", "BAD_MASK", "NO_CHORDS", "TOO_MANY_BARS", "BAD_BOUNDS", "NO_ROOM",
                                                            "NONFINITE"))
CONSTRAIN_STATUS_NAMES = ("ok", "bad_mask", "no_chords", "too_many_bars", "bad_bounds", "no_room", "nonfinite")
BARS_POLICY = {"exact": _GRAMMAR["MHG_BARS_EXACT"], "decodable": _GRAMMAR["MHG_BARS_DECODABLE"]}
COUNT_NAMES = ("bars", "notes", "through_eos")
# mirror of enum mhr_status (include/musehip_region.h)
REGION_OK, REGION_NOT_PLANNED, REGION_BAD_PLAN, REGION_NONFINITE, REGION_NO_ROOM = (
    ABI["musehip_region.h"].enums["MHR_" + n] for n in ("OK", "NOT_PLANNED", "BAD_PLAN", "NONFINITE", "NO_ROOM"))
REGION_STATUS_NAMES = ("ok", "not_planned", "bad_plan", "nonfinite", "no_room")
REGION_COUNT_NAMES = ("masked", "notes", "pads", "segments")


class ConstrainResult:
    """What constrain_tokens reports beside the tokens, all device tensors: status int32 [B] (CONSTRAIN_OK ...), path_score fp32 [B]
    (the score of the accepted string; 0 where the row is not OK), counts int32 [B, 3] = (Bars, notes, tokens of the note region
    through the EOS)."""

    def __init__(self, status, path_score, counts):
        self.status, self.path_score, self.counts = status, path_score, counts

    def vector(self):
        """device int64 [9]: rows per status (7), Bars and notes summed"""
        codes = torch.arange(len(CONSTRAIN_STATUS_NAMES), device=self.status.device, dtype=self.status.dtype)
        return torch.cat([(self.status.unsqueeze(1) == codes).sum(0), self.counts[:, :2].sum(0, dtype=torch.int64)])

    @staticmethod
    def describe(host):
        """the host list of a vector() (or of a sum of them) -> dict"""
        return {"rows": dict(zip(CONSTRAIN_STATUS_NAMES, (int(x) for x in host[:7]))), "bars": int(host[7]), "notes": int(host[8])}

    def summary(self):
        """one device -> host copy: {'rows': {'ok': n, 'bad_mask': n, ...}, 'bars', 'notes'}"""
        return self.describe(self.vector().cpu().tolist())


def _bars(bars, B, device):
    """'exact' | 'decodable' | (lo, hi) | int tensor [B, 2] -> (policy, bar_lo [B] or None, bar_hi [B] or None)"""
    if isinstance(bars, str):
        if bars not in BARS_POLICY:
            raise ValueError("bars: 'exact', 'decodable', a pair (lo, hi) or an int tensor [B, 2], got %r" % (bars,))
        return BARS_POLICY[bars], None, None
    if isinstance(bars, torch.Tensor):
        if tuple(bars.shape) != (B, 2):
            raise ValueError("bars: a tensor of per-row (lo, hi) is [B, 2] = [%d, 2], got %s" % (B, tuple(bars.shape)))
        require_device(bars)
        t = bars.to(device=device, dtype=torch.int32)
        return BARS_POLICY["exact"], t[:, 0].contiguous(), t[:, 1].contiguous()
    lo, hi = bars
    return (BARS_POLICY["exact"], torch.full((B,), int(lo), device=device, dtype=torch.int32),
            torch.full((B,), int(hi), device=device, dtype=torch.int32))


def constrain_rows(cls_score, cls_idx, input_ids, input_mask, bars="exact"):
    """mhg_constrain_rows on the two tables [B, L, 8] of ops.class_argmax (or any tables of that shape), the rows' input_ids and
    input_mask [B, L] -> (tokens int32 [B, L], ConstrainResult).  ONE launch whatever the batch."""
    require_device(cls_score, cls_idx, input_ids, input_mask)
    B, L = input_ids.shape
    if tuple(input_mask.shape) != (B, L) or tuple(cls_score.shape) != (B, L, 8) or tuple(cls_idx.shape) != (B, L, 8):
        raise ValueError("constrain_rows: tables [B, L, 8] and input_ids / input_mask [B, L]")
    if not 1 <= L <= lib().mh_batch_max_row():
        raise ValueError("constrain_rows: rows of 1..%d tokens, got %d" % (lib().mh_batch_max_row(), L))
    dev = input_ids.device
    policy, lo, hi = _bars(bars, B, dev)
    cls_score, cls_idx = cls_score.to(torch.float32).contiguous(), cls_idx.to(torch.int32).contiguous()
    ids, mask = input_ids.to(torch.int32).contiguous(), input_mask.to(torch.int32).contiguous()
    tokens = torch.empty(B, L, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    path_score = torch.empty(B, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 3, device=dev, dtype=torch.int32)
    need = lib().mhg_constrain_workspace_bytes(B, L)
    ws = torch.empty(need, device=dev, dtype=torch.uint8) if need else None
    check(lib().mhg_constrain_rows(ptr(cls_score), ptr(cls_idx), ptr(ids), ptr(mask), ptr(lo), ptr(hi), policy, ptr(tokens), ptr(status),
                                   ptr(path_score), ptr(counts), ptr(ws), need, B, L, current_stream()), "mhg_constrain_rows")
    return tokens, ConstrainResult(status, path_score, counts)


def class_tables(model, sample):
    """ops.class_argmax of the model's head on sample [B, L, E], in the model's logits_mode -> (cls_score, cls_idx) [B, L, 8]"""
    if model.logits_mode not in (1, 2):
        raise NotImplementedError
    w, b = model.lm_head.weight.detach(), model.lm_head.bias.detach()
    x = sample.to(torch.float32)
    if model.logits_mode == 2:                                        # |W_v|^2, as argmax_tokens finds it
        tied = w.data_ptr() == model.word_embedding.weight.data_ptr()
        cs, ci = ops.class_argmax(x, w, model.embedding_norms() if tied else ops.row_sqnorm(w), 2)
    else:
        cs, ci = ops.class_argmax(x, w, b, 1)
    shape = tuple(sample.shape[:-1]) + (8,)
    return cs.view(shape), ci.view(shape)


def constrain_tokens(model, sample, input_ids, input_mask, bars="exact"):
    """sample [B, L, E] (the last latent of a reverse loop) -> (tokens int64 [B, L], ConstrainResult): per row the best token
    sequence under the note grammar ( BAR | POSITION VELOCITY PITCH DURATION )* EOS PAD* in the note region [len_meta, L), the plain
    argmax in front of it.  bars: how many Bars a row may hold - 'exact' (as many as the chord part of its meta has bars),
    'decodable' (0 .. that + 1: every count the decoder restores), a pair (lo, hi) for every row, or an int tensor [B, 2].  A row
    whose status is not CONSTRAIN_OK equals model.argmax_tokens(sample) on that row.  Two launches."""
    cs, ci = class_tables(model, sample)
    dev = cs.device
    tokens, res = constrain_rows(cs, ci, input_ids.to(dev), input_mask.to(dev), bars)
    return tokens.long(), res


# ------------------------------------------------------------------------------------------------------------ infill regions
class RegionResult:
    """What constrain_region_tokens reports beside the tokens, all device tensors: status int32 [B] (REGION_OK ...), path_score fp32 [B]
    (the score of the accepted strings of the row's segments; 0 where the row is not OK), counts int32 [B, 4] = (masked slots, notes
    placed, pads placed, segments)."""

    def __init__(self, status, path_score, counts):
        self.status, self.path_score, self.counts = status, path_score, counts

    def vector(self):
        """device int64 [9]: rows per status (5), the four counts summed"""
        codes = torch.arange(len(REGION_STATUS_NAMES), device=self.status.device, dtype=self.status.dtype)
        return torch.cat([(self.status.unsqueeze(1) == codes).sum(0), self.counts.sum(0, dtype=torch.int64)])

    @staticmethod
    def describe(host):
        """the host list of a vector() (or of a sum of them) -> dict"""
        return {"rows": dict(zip(REGION_STATUS_NAMES, (int(x) for x in host[:5]))),
                **dict(zip(REGION_COUNT_NAMES, (int(x) for x in host[5:9])))}

    def summary(self):
        """one device -> host copy: {'rows': {'ok': n, 'not_planned': n, ...}, 'masked', 'notes', 'pads', 'segments'}"""
        return self.describe(self.vector().cpu().tolist())


def constrain_regions(cls_score, cls_idx, plan):
    """mhr_constrain_regions on the two tables [B, L, 8] of ops.class_argmax (or any tables of that shape) and an infill plan (anything
    with tokens / mask [B, L], status [B] and fields: utils/infill_util.InfillPlan) -> (tokens int32 [B, L], RegionResult).  ONE launch
    whatever the batch."""
    ptok, pmask, pstat = plan.tokens, plan.mask, plan.status
    require_device(cls_score, cls_idx, ptok, pmask, pstat)
    B, L = ptok.shape
    if tuple(pmask.shape) != (B, L) or tuple(pstat.shape) != (B,) or tuple(cls_score.shape) != (B, L, 8) or tuple(cls_idx.shape) != (B, L, 8):
        raise ValueError("constrain_regions: tables [B, L, 8], the plan's tokens / mask [B, L] and status [B]")
    if not 1 <= L <= lib().mh_batch_max_row():
        raise ValueError("constrain_regions: rows of 1..%d tokens, got %d" % (lib().mh_batch_max_row(), L))
    fields = int(plan.fields)
    if not 1 <= fields <= 15:
        raise ValueError("constrain_regions: the plan's fields are bits 1..15, got %d" % fields)
    dev = ptok.device
    cls_score, cls_idx = cls_score.to(torch.float32).contiguous(), cls_idx.to(torch.int32).contiguous()
    ptok, pmask, pstat = (t.to(torch.int32).contiguous() for t in (ptok, pmask, pstat))
    tokens = torch.empty(B, L, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    path_score = torch.empty(B, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    check(lib().mhr_constrain_regions(ptr(cls_score), ptr(cls_idx), ptr(ptok), ptr(pmask), ptr(pstat), fields, ptr(tokens), ptr(status),
                                      ptr(path_score), ptr(counts), B, L, current_stream()), "mhr_constrain_regions")
    return tokens, RegionResult(status, path_score, counts)


def constrain_region_tokens(model, sample, plan):
    """sample [B, L, E] (the last latent of a reverse loop run under the plan's mask) -> (tokens int64 [B, L], RegionResult): in every
    maximal run of plan.mask == 1 the best string of whole notes and pads (plan.fields == 15) or, per selected field slot, the best
    token of that field's class; the plain argmax everywhere else, and on every row whose status is not REGION_OK.  Two launches."""
    cs, ci = class_tables(model, sample)
    tokens, res = constrain_regions(cs, ci, plan)
    return tokens.long(), res
