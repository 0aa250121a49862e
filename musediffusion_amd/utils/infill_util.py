"""Infill: regenerate a bar range, or single note fields inside it, of pieces that are already token rows on the device
(csrc/infill.hip, include/musehip_infill.h).  Not in the reference, whose only edit re-noises the whole note region.

`plan_infill` turns (input_ids, input_mask, bars) into the row and the mask a reverse loop runs under - the interiors of the selected
bars, widened by `room` notes of pad slots each - and `splice_infill` brings the sampled row back: outside the region the original
tokens bit for bit, inside it only whole (position, velocity, pitch, duration) notes.  Two launches, no host loop over tokens, nothing
read back.  sampling.infill / sampling.run_infill drive the existing generate / modify paths with them."""
import torch

from .._lib import ABI, check, current_stream, lib, ptr

# mirror of enum mhi_status (include/musehip_infill.h)
INFILL_OK, INFILL_NO_EOS, INFILL_BAD_MASK, INFILL_BAD_RANGE, INFILL_OVERFLOW = (
    ABI["musehip_infill.h"].enums["MHI_" + n] for n in ("OK", "NO_EOS", "BAD_MASK", "BAD_RANGE", "OVERFLOW"))
INFILL_STATUS_MESSAGE = {
    INFILL_OK: "ok",
    INFILL_NO_EOS: "NO EOS TOKEN behind the prefix",
    INFILL_BAD_MASK: "input_mask is not m zeros followed by ones with 0 < m < L",
    INFILL_BAD_RANGE: "the bar range is not 0 <= lo < hi <= number of bars",
    INFILL_OVERFLOW: "the row has no room for the pad slots asked for (the EOS would fall off)",
}
# the short names, for users of this module alone (decode_util re-exports the INFILL_ ones beside its own decode statuses)
OK, NO_EOS, BAD_MASK, BAD_RANGE, OVERFLOW = INFILL_OK, INFILL_NO_EOS, INFILL_BAD_MASK, INFILL_BAD_RANGE, INFILL_OVERFLOW
STATUS_MESSAGE = INFILL_STATUS_MESSAGE

FIELDS = {"position": 1, "velocity": 2, "pitch": 4, "duration": 8, "all": 15}


def field_bits(fields):
    """a name of FIELDS, an iterable of names, or the bits themselves -> int in 1..15"""
    if isinstance(fields, str):
        fields = (fields,)
    if isinstance(fields, int) and not isinstance(fields, bool):
        bits = fields
    else:
        bits = 0
        for name in fields:
            if name not in FIELDS:
                raise ValueError("infill: unknown field %r (one of %s)" % (name, ", ".join(FIELDS)))
            bits |= FIELDS[name]
    if not 1 <= bits <= 15:
        raise ValueError("infill: fields must select at least one of position, velocity, pitch, duration (got %r)" % (fields,))
    return bits


def _as_device_i32(t):
    t = torch.as_tensor(t)
    if not t.is_cuda:
        t = t.to("cuda")
    return t.to(torch.int32).contiguous()


class InfillPlan:
    """tokens / mask [B, L] int32: what the reverse loop takes as input_ids / input_mask; prefix_mask [B, L]: the input_mask the plan was
    made from (the one to DECODE with: split_meta_midi counts the prefix by it); status [B] (INFILL_OK ...); info [B, 4] = (first region
    slot, one past the last, mask-1 slots, pad slots added); fields: the bits."""

    def __init__(self, tokens, mask, prefix_mask, status, info, fields):
        self.tokens, self.mask, self.prefix_mask, self.status, self.info, self.fields = tokens, mask, prefix_mask, status, info, fields


def plan_infill(input_ids, input_mask, bars, room=0, fields="all"):
    """input_ids / input_mask [B, L]; bars = (lo, hi) for every row or an int tensor [B, 2]: bars lo <= k < hi, counted from the first
    BAR behind the prefix; room: notes of space added to every selected bar (whole notes only) -> InfillPlan.  A row that cannot be
    planned keeps its tokens, gets an all-zero mask and says why in status."""
    bits = field_bits(fields)
    room = int(room)
    if room < 0 or (room and bits != 15):
        raise ValueError("infill: room >= 0, and only with fields='all' (got room = %d, fields = %d)" % (room, bits))
    tokens, prefix_mask = _as_device_i32(input_ids), _as_device_i32(input_mask)
    if tokens.dim() != 2 or prefix_mask.shape != tokens.shape:
        raise ValueError("infill: input_ids and input_mask must both be [B, L]")
    B, L = tokens.shape
    dev = tokens.device
    if torch.is_tensor(bars):
        if tuple(bars.shape) != (B, 2):
            raise ValueError("infill: bars is (lo, hi) or an int tensor [B, 2], got %s" % (tuple(bars.shape),))
        lohi = bars.to(dev).to(torch.int32).t().contiguous()          # [2, B]
    else:
        lo, hi = bars
        lohi = torch.tensor([[int(lo)], [int(hi)]], dtype=torch.int32).expand(2, B).contiguous().to(dev)
    out_tokens, out_mask = torch.empty_like(tokens), torch.empty_like(tokens)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    info = torch.empty(B, 4, device=dev, dtype=torch.int32)
    check(lib().mhi_infill_plan(ptr(tokens), ptr(prefix_mask), ptr(lohi[0]), ptr(lohi[1]), room, bits, ptr(out_tokens), ptr(out_mask),
                                ptr(status), ptr(info), B, L, current_stream()), "mhi_infill_plan")
    return InfillPlan(out_tokens, out_mask, prefix_mask, status, info, bits)


def splice_infill(plan, sampled):
    """sampled [B, L]: the tokens a sampler returned for {'input_ids': plan.tokens, 'input_mask': plan.mask} -> (tokens [B, L] int32,
    counts [B, 4] int32 = (region tokens kept, pads dropped, other dropped or rejected, kept slots that changed - field mode))."""
    sampled = _as_device_i32(sampled)
    if sampled.shape != plan.tokens.shape or sampled.device != plan.tokens.device:
        raise ValueError("infill: sampled must be the plan's [B, L] on the plan's device")
    B, L = sampled.shape
    out = torch.empty_like(plan.tokens)
    counts = torch.empty(B, 4, device=out.device, dtype=torch.int32)
    check(lib().mhi_infill_splice(ptr(sampled), ptr(plan.tokens), ptr(plan.mask), ptr(plan.status), plan.fields, ptr(out), ptr(counts), B,
                                  L, current_stream()), "mhi_infill_splice")
    return out, counts


class InfillResult:
    """What sampling.infill reports beside the tokens: the plan, counts [B, 4] and status [B] (device tensors); rounding: the
    grammar_util.RegionResult of infill(rounding='region'), else None."""

    COUNT_NAMES = ("kept", "pads", "other", "changed")

    def __init__(self, plan, counts, rounding=None):
        self.plan, self.counts, self.status, self.rounding = plan, counts, plan.status, rounding

    def vector(self):
        """device int64 [9]: rows per status (5), the four counts summed"""
        codes = torch.arange(len(INFILL_STATUS_MESSAGE), device=self.status.device, dtype=self.status.dtype)
        return torch.cat([(self.status.unsqueeze(1) == codes).sum(0), self.counts.sum(0, dtype=torch.int64)])

    @staticmethod
    def describe(host):
        """the host list of a vector() (or of a sum of them) -> dict"""
        names = ("ok", "no_eos", "bad_mask", "bad_range", "overflow")
        return {"rows": dict(zip(names, (int(x) for x in host[:5]))), **dict(zip(InfillResult.COUNT_NAMES, (int(x) for x in host[5:9])))}

    def summary(self):
        """one device -> host copy: {'rows': {'ok': n, 'no_eos': n, ...}, 'kept', 'pads', 'other', 'changed'}"""
        return self.describe(self.vector().cpu().tolist())
