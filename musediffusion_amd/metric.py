"""MSIM / 1NNC of MuseDiffusion/metric.py:4-117 for whole batches on the device.

The reference walks every sequence token by token in Python (`get_vectors`) and then multiplies three small similarity
matrices; here one kernel launch extracts the [32 rhythm | 12 melody | 12 harmony] features of all sequences and the
three similarity matrices come from the library's exact-fp32 MFMA GEMM.

Additions without a reference counterpart: `nearest` / `ONNC_sets` (the fused 1-NN kernel, csrc/evaluate.hip) and `pair_stats` /
`diversity` (sum and counts over all pairs of a set, csrc/pairstats.hip); neither writes the similarity matrix.  `harmony_counts` /
`Controllability_Harmony` (csrc/harmony.hip) are CH, the control metric of the ComMU paper the reference never wrote: do the notes of
a decoded piece fit the chord progression it was conditioned on.  `structure_counts` (csrc/structure.hip) are the per-bar counts
behind H1 / H4 (pitch-class entropy of 1-bar and 4-bar windows) and GS (groove similarity) of the MusDr set: is a piece shaped like
music over time.  `interplay_counts` (csrc/arrange.hip) looks at the rows of one song together: which intervals sound between the
tracks, for how long, and which track lies below.

Where this module differs from the reference, on purpose (pinned by tests/test_batch_matrix_gpu.py):
  * get_vectors never raises: status 1 = no BAR token (the reference: IndexError), 2 = a malformed note group or a row that ends
    without terminator (ValueError / IndexError); the vectors of a flagged row mean nothing.
  * a row with no position token between its first BAR and its EOS ([2, 1]) makes the reference read an unassigned variable
    (UnboundLocalError); here it gets status 0, flat rhythm and melody vectors and, like any row without notes (chords only), the
    0 / 0 = NaN harmony vector the reference returns for those.
  * Controllability_Pitch judges a range token (meta[3]) outside 630..637 by the nearest range (below 631 as 631, above 637 as
    637) where the reference raises KeyError; a row without pitch tokens counts as wrong, as the reference's NaN mean does."""
import numpy as np
import torch

from ._lib import ABI, EXTENSION_ABI, check, current_stream, lib, ptr, require_device


def get_vectors(tokens, lengths=None, note_len=128, return_status=False):
    """[B, L] int note tokens (from anywhere before the first BAR) -> fp32 [B, 56]; metric.py:4-71 for every row at once."""
    require_device(tokens, lengths)
    tokens = tokens.to(torch.int32).contiguous()
    B, L = tokens.shape
    lengths = None if lengths is None else lengths.to(torch.int32).contiguous()
    out = torch.empty(B, 56, device=tokens.device, dtype=torch.float32)
    status = torch.empty(B, device=tokens.device, dtype=torch.int32)
    check(lib().mh_msim_vectors(ptr(tokens), ptr(lengths), ptr(out), ptr(status), B, L, float(note_len), current_stream()), "mh_msim_vectors")
    return (out, status) if return_status else out


def _gram(a, b):
    """a b^T for [Ba, C] x [Bb, C] fp32 on the library's exact-fp32 MFMA GEMM (C zero-padded to the kernel's K granule of 16)."""
    from . import ops
    C = a.shape[1]
    Cp = (C + 15) // 16 * 16
    pad = lambda t: ops.cast_pad(t.contiguous(), Cp, ops.MH_F32)
    return ops.gemm_bias_act(pad(a), pad(b), None, None, None, ops.MH_F32, out_f32=True, N=b.shape[0], K=Cp)


def _similarity(vec_a, vec_b):
    """metric.py:96-104: rhythm x melody x harmony similarity matrices, multiplied element-wise"""
    r = _gram(vec_a[:, :32], vec_b[:, :32])
    m = _gram(vec_a[:, 32:44], vec_b[:, 32:44])
    h = _gram(vec_a[:, 44:], vec_b[:, 44:])
    return r * m * h


def MSIM(tokens1, tokens2, lengths1=None, lengths2=None):
    """metric.py:74-83 for paired batches: msim[b] = <r1,r2> <m1,m2> <h1,h2>"""
    a, b = get_vectors(tokens1, lengths1), get_vectors(tokens2, lengths2)
    return (a[:, :32] * b[:, :32]).sum(-1) * (a[:, 32:44] * b[:, 32:44]).sum(-1) * (a[:, 44:] * b[:, 44:]).sum(-1)


def ONNC(tokens, lengths=None, return_MSIM=False, return_mostsim=False):
    """metric.py:86-117: first half of the batch = ground truth, second half = generated; 1NNC from the MSIM matrix."""
    vec = get_vectors(tokens, lengths)
    sim = _similarity(vec, vec)
    sim.fill_diagonal_(0)
    most = torch.argmax(sim, dim=1)
    half = vec.shape[0] // 2
    onnc = ((most[:half] < half).sum() + (most[half:] >= half).sum()) / vec.shape[0]
    extra = ([sim] if return_MSIM else []) + ([most] if return_mostsim else [])
    return onnc if not extra else [onnc] + extra


PITCH_RANGE = {631: (3, 38), 632: (39, 50), 633: (51, 62), 634: (63, 74), 635: (75, 86), 636: (87, 98), 637: (99, 130)}


def _counts(metas, tokens, lengths):
    require_device(metas, tokens, lengths)
    tokens = tokens.to(torch.int32).contiguous()
    metas = metas.to(torch.int32).contiguous()
    B, L = tokens.shape
    lengths = None if lengths is None else lengths.to(torch.int32).contiguous()
    out = torch.empty(B, 4, device=tokens.device, dtype=torch.int32)
    check(lib().mh_controllability_counts(ptr(tokens), ptr(lengths), ptr(metas), metas.shape[1], ptr(out), B, L, current_stream()),
          "mh_controllability_counts")
    return out


def Controllability_Pitch(metas, tokens, lengths=None):
    """metric.py:131-148 on device batches -> (total rows, rows whose mean pitch leaves the range its meta asks for)"""
    c = _counts(metas, tokens, lengths)
    rng = metas[:, 3].long()
    lo = torch.tensor([PITCH_RANGE.get(k, (0, 0))[0] for k in range(631, 638)], device=tokens.device, dtype=torch.float32)
    hi = torch.tensor([PITCH_RANGE.get(k, (0, 0))[1] for k in range(631, 638)], device=tokens.device, dtype=torch.float32)
    idx = (rng - 631).clamp(0, 6)
    mean = c[:, 0].float() / c[:, 1].clamp(min=1).float()
    wrong = (rng != 630) & ~((lo[idx] <= mean) & (mean <= hi[idx]))
    return metas.shape[0], int(wrong.sum())


def Controllability_Velocity(metas, tokens, lengths=None):
    """metric.py:151-168 -> (velocity tokens of the rows with a bounded maximum, those outside their meta's [min, max])"""
    c = _counts(metas, tokens, lengths)
    use = (metas[:, 8].long() - 524) != 130
    return int(c[use, 2].sum()), int(c[use, 3].sum())


# ------------------------------------------------------------------------------------------ fused 1-NN (csrc/evaluate.hip), additions
def _mask_i32(mask, n, device):
    if mask is None:
        return None
    require_device(mask)
    assert mask.shape == (n,), "a validity mask holds one entry per row"
    return (mask != 0).to(device=device, dtype=torch.int32).contiguous()


def nearest(vec, keys=None, valid=None, keys_valid=None, return_values=False, return_sim=False):
    """For every row of vec [nq, 56] (get_vectors' layout) the index of its most similar row of keys [nk, 56] under the MSIM similarity
    of metric.py:100-103, by torch.argmax's rule (lowest index among equals, the first NaN beats every number), in ONE launch that
    never writes the nq x nk matrix (mhe_msim_nearest, include/musehip_eval.h).  keys=None is the self mode of metric.py:104-105: the
    keys are vec itself, `valid` masks both sides and sim(i, i) counts as 0.  valid / keys_valid: [nq] / [nk] masks (bool or int), a
    masked key is skipped and a masked query row, or one without a candidate, gets -1 (value 0).  Indices are into the rows as given.
    Returns int32 most [nq]; with return_values also the fp32 similarity of the winner; with return_sim also the [nq, nk] matrix (small
    sets and tests: NaN where a masked row or column was skipped)."""
    require_device(vec, keys)
    self_mode = keys is None
    assert not (self_mode and keys_valid is not None), "self mode: `valid` masks both sides"
    vec = vec.to(torch.float32).contiguous()
    keys = vec if self_mode else keys.to(device=vec.device, dtype=torch.float32).contiguous()
    assert vec.dim() == 2 and keys.dim() == 2 and vec.shape[1] == 56 and keys.shape[1] == 56, "rows of 56 values (32 | 12 | 12)"
    nq, nk = vec.shape[0], keys.shape[0]
    qv = _mask_i32(valid, nq, vec.device)
    kv = qv if self_mode else _mask_i32(keys_valid, nk, vec.device)
    most = torch.empty(nq, device=vec.device, dtype=torch.int32)
    best = torch.empty(nq, device=vec.device, dtype=torch.float32) if return_values else None
    sim = torch.full((nq, nk), float("nan"), device=vec.device, dtype=torch.float32) if return_sim else None
    check(lib().mhe_msim_nearest(ptr(vec), nq, ptr(keys), nk, ptr(qv), ptr(kv), int(self_mode), ptr(most), ptr(best), ptr(sim), current_stream()),
          "mhe_msim_nearest")
    extra = ([best] if return_values else []) + ([sim] if return_sim else [])
    return most if not extra else [most] + extra


def ONNC_sets(gt_tokens, gen_tokens, gt_lengths=None, gen_lengths=None, valid=None, return_mostsim=False):
    """The 1NNC of metric.py:83-117 with the two halves as two arguments: gt_tokens [B1, L1] the ground truth, gen_tokens [B2, L2] the
    generated set.  The get_vectors rows of both go into one [B1 + B2, 56] buffer and one `nearest` call (self mode) classifies every row:
        onnc = (#valid gt rows whose nearest is a gt row + #valid generated rows whose nearest is a generated row) / #valid rows
    as an fp32 device scalar (NaN when no row is valid); nothing here syncs with the host.  `valid`: None, one [B] mask for equal
    halves - applied to both, as run/sample.py:247-252 drops a row from both lists - or a pair (gt mask [B1], generated mask [B2]) for
    sets of unequal size (a validation split against a generated set).
    `most` (return_mostsim) holds indices into the UNCOMPACTED concatenation [gt | generated], -1 for a masked row, where the
    reference's most_sim indexes the compacted list of valid rows; which half each index falls into, and so the count, is the same."""
    B1, B2 = gt_tokens.shape[0], gen_tokens.shape[0]
    if gt_tokens.shape[1] == gen_tokens.shape[1] and (gt_lengths is None) == (gen_lengths is None):
        # rows of one width: the feature kernel is per row and latency bound, so one launch over [gt | generated] gives the same
        # [B1 + B2, 56] buffer as two launches and a cat, in half the time
        lengths = None if gt_lengths is None else torch.cat([gt_lengths.to(torch.int32), gen_lengths.to(torch.int32)])
        vec = get_vectors(torch.cat([gt_tokens.to(torch.int32), gen_tokens.to(torch.int32)]), lengths)
    else:
        vec = torch.cat([get_vectors(gt_tokens, gt_lengths), get_vectors(gen_tokens, gen_lengths)])
    if valid is None:
        mask = None
    elif isinstance(valid, (tuple, list)):
        mask = torch.cat([(valid[0] != 0).reshape(B1), (valid[1] != 0).reshape(B2)])
    else:
        assert B1 == B2, "one mask serves both halves only when they are of equal size: pass (gt_valid, gen_valid)"
        mask = torch.cat([(valid != 0).reshape(B1)] * 2)
    most = nearest(vec, valid=mask)
    own = torch.cat([most[:B1] < B1, most[B1:] >= B1]) & (most >= 0)
    total = mask.sum() if mask is not None else B1 + B2
    onnc = own.sum() / total
    return [onnc, most] if return_mostsim else onnc


def controllability_counts(metas, tokens, lengths=None, valid=None):
    """Controllability_Pitch and Controllability_Velocity as device scalars: int64 [4] = (rows, rows whose mean pitch leaves its range,
    velocity tokens of the rows with a bounded maximum, those outside [min, max]), over the rows where `valid` ([B], default all) is
    set.  The rules are those of the two functions above; nothing syncs with the host."""
    c = _counts(metas, tokens, lengths)
    v = torch.ones(metas.shape[0], device=tokens.device, dtype=torch.bool) if valid is None else (valid != 0)
    rng = metas[:, 3].long()
    idx = (rng - 631).clamp(0, 6)
    lo = torch.where(idx == 0, 3, 27 + 12 * idx).float()        # PITCH_RANGE as arithmetic: no table to copy to the device
    hi = torch.where(idx == 6, 130, 38 + 12 * idx).float()
    mean = c[:, 0].float() / c[:, 1].clamp(min=1).float()
    wrong = (rng != 630) & ~((lo <= mean) & (mean <= hi)) & v
    use = ((metas[:, 8].long() - 524) != 130) & v
    zero = torch.zeros((), device=tokens.device, dtype=torch.int64)
    return torch.stack([v.sum(), wrong.sum(), torch.where(use, c[:, 2].long(), zero).sum(), torch.where(use, c[:, 3].long(), zero).sum()])


# ------------------------------------------------------------------------------------------ pair statistics (csrc/pairstats.hip), additions
class PairStats:
    """Per query row over its counted pairs (include/musehip_stats.h): sum fp64 [nq] of the non-NaN similarities, count int32 [nq] of
    them, nan int32 [nq] of the NaN ones, above int32 [nq] = how many of the counted similarities reach the threshold (None without one)."""

    def __init__(self, sum, count, nan, above):
        self.sum, self.count, self.nan, self.above = sum, count, nan, above


def _group_i32(groups, n, device):
    if groups is None:
        return None
    require_device(groups)
    assert groups.shape == (n,), "a group id per row"
    return groups.to(device=device, dtype=torch.int32).contiguous()


def pair_stats(vec, keys=None, valid=None, keys_valid=None, groups=None, keys_groups=None, threshold=None):
    """Sum and counts of the MSIM similarities of every row of vec [nq, 56] with the rows of keys [nk, 56], in ONE launch that never
    writes the nq x nk matrix (mhs_msim_pair_stats): the similarity is bit for bit the one `nearest` selects from.  The conventions
    are `nearest`'s: keys=None is the self mode (the keys are vec itself, `valid` and `groups` serve both sides) - but here a row is no
    pair with itself: the diagonal is left out, not counted as 0.  valid / keys_valid: [nq] / [nk] masks (bool or int); a masked key is
    skipped, a masked query row gets zeros.  groups / keys_groups: integer ids [nq] / [nk], only pairs of equal ids count (None: one
    group, id 0).  threshold: a Python float; `above` counts the similarities >= it in fp32.  Returns a PairStats; nothing syncs."""
    require_device(vec, keys)
    self_mode = keys is None
    assert not (self_mode and (keys_valid is not None or keys_groups is not None)), "self mode: `valid` and `groups` serve both sides"
    vec = vec.to(torch.float32).contiguous()
    keys = vec if self_mode else keys.to(device=vec.device, dtype=torch.float32).contiguous()
    assert vec.dim() == 2 and keys.dim() == 2 and vec.shape[1] == 56 and keys.shape[1] == 56, "rows of 56 values (32 | 12 | 12)"
    nq, nk = vec.shape[0], keys.shape[0]
    qv = _mask_i32(valid, nq, vec.device)
    kv = qv if self_mode else _mask_i32(keys_valid, nk, vec.device)
    qg = _group_i32(groups, nq, vec.device)
    kg = qg if self_mode else _group_i32(keys_groups, nk, vec.device)
    total = torch.empty(nq, device=vec.device, dtype=torch.float64)
    count, nan = (torch.empty(nq, device=vec.device, dtype=torch.int32) for _ in range(2))
    above = torch.empty(nq, device=vec.device, dtype=torch.int32) if threshold is not None else None
    check(lib().mhs_msim_pair_stats(ptr(vec), nq, ptr(keys), nk, ptr(qv), ptr(kv), ptr(qg), ptr(kg), int(self_mode),
                                    float("nan") if threshold is None else float(threshold), ptr(total), ptr(count), ptr(nan), ptr(above),
                                    current_stream()), "mhs_msim_pair_stats")
    return PairStats(total, count, nan, above)


def diversity(vec, valid=None, groups=None):
    """How different the rows of a set are from each other: (1 - sum of all counted similarities / number of counted pairs, the
    per-row mean similarity sum / count), both float64 on the device - a scalar and [n]; NaN where nothing was counted.  One
    pair_stats launch in self mode; nothing syncs with the host."""
    st = pair_stats(vec, valid=valid, groups=groups)
    return 1.0 - st.sum.sum() / st.count.sum().double(), st.sum / st.count.double()


# ------------------------------------------------------------------------------------------ chord fit (csrc/harmony.hip), additions
# mirror of enum mhh_status (include/musehip_harmony.h)
HARMONY_OK, HARMONY_MASKED, HARMONY_BAD_META, HARMONY_BAD_COUNTS = (ABI["musehip_harmony.h"].enums["MHH_" + n] for n in ("OK", "MASKED", "BAD_META", "BAD_COUNTS"))
HARMONY_COUNT_NAMES = ("notes", "judged", "chord_tones", "scale_tones", "ticks", "judged_ticks", "chord_tone_ticks", "bars_used")
HARMONY_MAX_NOTES, HARMONY_MAX_CHORDS, HARMONY_MAX_BARS = 32768, 4096, 512


class HarmonyCounts:
    """Device results of one batch (include/musehip_harmony.h): counts int32 [B, 8] in HARMONY_COUNT_NAMES order, status int32 [B]
    (HARMONY_OK ...; a row that is not OK has zeros everywhere), bars int32 [B, max_bars, 4] = (notes, judged, chord tones, scale
    tones) of the notes that start in each bar, or None, hist int32 [B, 12] = notes per pitch class, or None."""

    def __init__(self, counts, status, bars, hist):
        self.counts, self.status, self.bars, self.hist = counts, status, bars, hist


def harmony_counts_raw(notes, chords, counts3, meta, valid=None, max_bars=0, return_hist=False):
    """mhh_harmony_counts on the five tensors a decode leaves: notes [B, max_notes, 4] = (start tick, end tick, pitch, velocity),
    chords [B, max_chords, 2] = (tick, chord token), counts3 [B, 3] = (notes, chords, -), meta [B, 11], valid [B] or None (every
    row) -> HarmonyCounts.  Does every note fit the chord in force at its onset and the scale of the piece's key: the rule is the
    header's.  ONE launch whatever the batch; nothing syncs with the host."""
    require_device(notes, chords, counts3, meta, valid)
    max_bars = int(max_bars)
    if notes.dim() != 3 or notes.shape[2] != 4 or chords.dim() != 3 or chords.shape[2] != 2 or chords.shape[0] != notes.shape[0]:
        raise ValueError("harmony_counts: notes [B, max_notes, 4] and chords [B, max_chords, 2]")
    B, max_notes, max_chords = notes.shape[0], notes.shape[1], chords.shape[1]
    if tuple(counts3.shape) != (B, 3) or tuple(meta.shape) != (B, 11):
        raise ValueError("harmony_counts: counts [B, 3] and meta [B, 11]")
    if not (1 <= max_notes <= HARMONY_MAX_NOTES and 1 <= max_chords <= HARMONY_MAX_CHORDS and 0 <= max_bars <= HARMONY_MAX_BARS):
        raise ValueError("harmony_counts: max_notes in 1..%d, max_chords in 1..%d, max_bars in 0..%d (got %d, %d, %d)" % (
            HARMONY_MAX_NOTES, HARMONY_MAX_CHORDS, HARMONY_MAX_BARS, max_notes, max_chords, max_bars))
    dev = notes.device
    notes, chords, counts3, meta = (t.to(torch.int32).contiguous() for t in (notes, chords, counts3, meta))
    valid = _mask_i32(valid, B, dev)
    counts = torch.empty(B, 8, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    hist = torch.empty(B, 12, device=dev, dtype=torch.int32) if return_hist else None
    bars = torch.empty(B, max_bars, 4, device=dev, dtype=torch.int32) if max_bars else None
    check(lib().mhh_harmony_counts(ptr(notes), ptr(chords), ptr(counts3), ptr(meta), ptr(valid), ptr(counts), ptr(hist), ptr(bars), ptr(status),
                                   B, max_notes, max_chords, max_bars, current_stream()), "mhh_harmony_counts")
    return HarmonyCounts(counts, status, bars, hist)


def harmony_counts(decoded, valid=None, max_bars=0, return_hist=False):
    """harmony_counts_raw on a DecodedBatch (utils.decode_util.decode_tokens); valid defaults to the rows that decoded
    (decoded.status == OK: the lists of the others hold nothing)."""
    if valid is None:
        valid = decoded.status == 0
    return harmony_counts_raw(decoded.notes, decoded.chords, decoded.counts, decoded.meta, valid, max_bars, return_hist)


def Controllability_Harmony(decoded, valid=None):
    """CH, the third control metric beside Controllability_Pitch / _Velocity -> (judged notes, judged notes that are no tone of the
    chord in force at their onset) of the valid rows, as Python ints (total, wrong)."""
    c = harmony_counts(decoded, valid).counts[:, 1:3].sum(0, dtype=torch.int64).cpu().tolist()
    return int(c[0]), int(c[0] - c[1])


# ------------------------------------------------------------------------------------------ structure (csrc/structure.hip), additions
# mirror of enum mhm_status (include/musehip_structure.h)
STRUCTURE_OK, STRUCTURE_MASKED, STRUCTURE_BAD_META, STRUCTURE_BAD_COUNTS = (ABI["musehip_structure.h"].enums["MHM_" + n] for n in ("OK", "MASKED", "BAD_META", "BAD_COUNTS"))
STRUCTURE_COUNT_NAMES = ("notes", "skipped", "bars_used", "bars_with_notes", "pitch_classes", "distinct_pitches", "lowest_pitch",
                         "highest_pitch", "onsets", "pairs", "diff", "slots_per_bar", "windows_1", "windows_4", "reserved_0", "reserved_1")
STRUCTURE_BAR_NAMES = ("notes", "onset_mask", "lowest_pitch", "highest_pitch") + tuple("pitch_class_%d" % p for p in range(12))
STRUCTURE_MAX_NOTES, STRUCTURE_MAX_BARS = 32768, 512

_XLOG2X_TABLES = {}


def xlog2x_host(n):
    """numpy float64 [n + 1]: k log2 k, entry 0 = 0 - the table mhm_structure_counts takes its entropies from"""
    k = np.arange(int(n) + 1, dtype=np.float64)
    table = np.zeros(int(n) + 1, np.float64)
    table[1:] = k[1:] * np.log2(k[1:])
    return table


def xlog2x_table(n, device):
    """xlog2x_host(n) as a float64 tensor on `device`, cached per device and size (uploaded once, not per call)"""
    key = (int(n), str(device))
    hit = _XLOG2X_TABLES.get(key)
    if hit is None:
        if len(_XLOG2X_TABLES) > 64:
            _XLOG2X_TABLES.clear()
        hit = _XLOG2X_TABLES[key] = torch.from_numpy(xlog2x_host(n)).to(device)
    return hit


class StructureCounts:
    """Device results of one batch (include/musehip_structure.h): counts int32 [B, 16] in STRUCTURE_COUNT_NAMES order, entropy float64
    [B, 2] = (sum of the pitch-class entropy over the 1-bar windows, over the 4-bar windows; divide by counts[:, 12:14]), status int32
    [B] (STRUCTURE_OK ...; a row that is not OK has zeros everywhere), bars int32 [B, max_bars, 16] in STRUCTURE_BAR_NAMES order, or
    None."""

    def __init__(self, counts, entropy, status, bars):
        self.counts, self.entropy, self.status, self.bars = counts, entropy, status, bars


def structure_counts_raw(notes, counts3, meta, valid=None, max_bars=64, return_bars=False):
    """mhm_structure_counts on the tensors a decode leaves: notes [B, max_notes, 4] = (start tick, end tick, pitch, velocity), counts3
    [B, 3] = (notes, -, -), meta [B, 11], valid [B] or None (every row) -> StructureCounts.  Per bar of a sixteenth-note grid: notes,
    pitch-class histogram, onset mask, pitch range; per row the entropy sums of the 1-bar and 4-bar windows and the pairwise distance
    of the bars' onset masks: the rule is the header's.  Notes that start at or behind bar max_bars are skipped (counts[:, 1]).  ONE
    launch whatever the batch; nothing syncs with the host."""
    max_bars = int(max_bars)
    if notes.dim() != 3 or notes.shape[2] != 4:
        raise ValueError("structure_counts: notes [B, max_notes, 4]")
    B, max_notes = notes.shape[0], notes.shape[1]
    if tuple(counts3.shape) != (B, 3) or tuple(meta.shape) != (B, 11):
        raise ValueError("structure_counts: counts [B, 3] and meta [B, 11]")
    if not (1 <= max_notes <= STRUCTURE_MAX_NOTES and 1 <= max_bars <= STRUCTURE_MAX_BARS):
        raise ValueError("structure_counts: max_notes in 1..%d, max_bars in 1..%d (got %d, %d)" % (
            STRUCTURE_MAX_NOTES, STRUCTURE_MAX_BARS, max_notes, max_bars))
    if B < 1:
        raise ValueError("structure_counts: an empty batch")
    require_device(notes, counts3, meta, valid)
    dev = notes.device
    notes, counts3, meta = (t.to(torch.int32).contiguous() for t in (notes, counts3, meta))
    valid = _mask_i32(valid, B, dev)
    table = xlog2x_table(max_notes, dev)
    counts = torch.empty(B, 16, device=dev, dtype=torch.int32)
    entropy = torch.empty(B, 2, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    bars = torch.empty(B, max_bars, 16, device=dev, dtype=torch.int32) if return_bars else None
    check(lib().mhm_structure_counts(ptr(notes), ptr(counts3), ptr(meta), ptr(valid), ptr(table), ptr(counts), ptr(entropy), ptr(bars),
                                     ptr(status), B, max_notes, max_bars, current_stream()), "mhm_structure_counts")
    return StructureCounts(counts, entropy, status, bars)


def structure_counts(decoded, valid=None, max_bars=64, return_bars=False):
    """structure_counts_raw on a DecodedBatch (utils.decode_util.decode_tokens); valid defaults to the rows that decoded
    (decoded.status == OK: the lists of the others hold nothing)."""
    if valid is None:
        valid = decoded.status == 0
    return structure_counts_raw(decoded.notes, decoded.counts, decoded.meta, valid, max_bars, return_bars)


# ------------------------------------------------------------------------------------------ interplay (csrc/arrange.hip), additions
# mirror of enum mha_status (include/musehip_arrange.h)
INTERPLAY_OK, INTERPLAY_MASKED, INTERPLAY_BAD_COUNTS, INTERPLAY_BAD_SHIFT, INTERPLAY_MIXED = (
    ABI["musehip_arrange.h"].enums["MHA_" + n] for n in ("OK", "MASKED", "BAD_COUNTS", "BAD_SHIFT", "MIXED"))
INTERPLAY_COUNT_NAMES = ("notes", "skipped", "partners", "accompanied", "reserved_0", "reserved_1", "reserved_2", "reserved_3")
INTERPLAY_COLUMN_NAMES = tuple("interval_class_%d" % i for i in range(7)) + ("below", "above")
INTERPLAY_MAX_NOTES, INTERPLAY_MAX_SHIFT = 32768, 1 << 29
DRUMS_INST = 648                                              # the inst token (meta[5]) of the drum group: its note numbers are no pitches


class InterplayCounts:
    """Device results of one batch (include/musehip_arrange.h): status int32 [B] (INTERPLAY_OK ...; a row that is not OK has zeros
    everywhere), counts int32 [B, 8] in INTERPLAY_COUNT_NAMES order, pairs and ticks int64 [B, 9] in INTERPLAY_COLUMN_NAMES order: the
    pairs (this row's note, a partner's note) that sound together and their common ticks, at most 65535 a pair."""

    def __init__(self, status, counts, pairs, ticks):
        self.status, self.counts, self.pairs, self.ticks = status, counts, pairs, ticks


def interplay_counts_raw(notes, counts3, meta, valid=None, song=None, shift=None):
    """mha_interplay_counts on the tensors a decode leaves: notes [B, max_notes, 4] = (start tick, end tick, pitch, velocity), counts3
    [B, 3] = (notes, -, -), meta [B, 11], valid [B] or None (every row), song [B] int group ids or None (one song), shift [B] ticks
    added to a row's notes or None -> InterplayCounts.  The rows of one song are partners; the rule is the header's.  ONE launch
    whatever the batch; nothing syncs with the host."""
    if notes.dim() != 3 or notes.shape[2] != 4:
        raise ValueError("interplay_counts: notes [B, max_notes, 4]")
    B, max_notes = notes.shape[0], notes.shape[1]
    if tuple(counts3.shape) != (B, 3) or tuple(meta.shape) != (B, 11):
        raise ValueError("interplay_counts: counts [B, 3] and meta [B, 11]")
    for name, t in (("song", song), ("shift", shift)):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError("interplay_counts: %s holds one entry per row" % name)
    if not 1 <= max_notes <= INTERPLAY_MAX_NOTES or B * max_notes > 1 << 31:
        raise ValueError("interplay_counts: max_notes in 1..%d and B * max_notes <= 2^31 (got %d, %d)" % (INTERPLAY_MAX_NOTES, max_notes, B))
    if B < 1:
        raise ValueError("interplay_counts: an empty batch")
    require_device(notes, counts3, meta, valid, song, shift)
    dev = notes.device
    notes, counts3, meta = (t.to(torch.int32).contiguous() for t in (notes, counts3, meta))
    valid = _mask_i32(valid, B, dev)
    song, shift = (None if t is None else t.to(device=dev, dtype=torch.int32).contiguous() for t in (song, shift))
    counts = torch.empty(B, 8, device=dev, dtype=torch.int32)
    pairs = torch.empty(B, 9, device=dev, dtype=torch.int64)
    ticks = torch.empty(B, 9, device=dev, dtype=torch.int64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().mha_interplay_counts(ptr(notes), ptr(counts3), ptr(meta), ptr(valid), ptr(song), ptr(shift), ptr(counts), ptr(pairs),
                                     ptr(ticks), ptr(status), B, max_notes, current_stream()), "mha_interplay_counts")
    return InterplayCounts(status, counts, pairs, ticks)


def interplay_counts(decoded, song, valid=None, shift=None, pitched_only=True):
    """interplay_counts_raw on a DecodedBatch (utils.decode_util.decode_tokens) whose rows `song` [B] groups into songs; valid
    defaults to the rows that decoded (decoded.status == OK: the lists of the others hold nothing); shift: ticks per row, as
    utils.arrange_util.align_shift makes them; pitched_only: the rows of the drum group (meta[5] == 648) are masked - a drum note
    number is not a pitch, so no interval with it means anything."""
    if valid is None:
        valid = decoded.status == 0
    if pitched_only:
        valid = (valid != 0) & (decoded.meta[:, 5] != DRUMS_INST)
    return interplay_counts_raw(decoded.notes, decoded.counts, decoded.meta, valid, song, shift)


# ------------------------------------------------------------------- choosing among candidates (csrc/choose.hip), additions
# mirror of enum mhac_status and enum mhac_limit (include/musehip_choose.h, an extension family: _lib.EXTENSION_HEADERS)
_CHOOSE = EXTENSION_ABI["musehip_choose.h"].enums
CHOOSE_OK, CHOOSE_PARTIAL, CHOOSE_EMPTY, CHOOSE_BAD_SCORE = (_CHOOSE["MHAC_" + n] for n in ("OK", "PARTIAL", "EMPTY", "BAD_SCORE"))
CHOOSE_MAX_TRACKS, CHOOSE_MAX_CANDIDATES, CHOOSE_MAX_COMBINATIONS = (
    _CHOOSE["MHAC_MAX_" + n] for n in ("TRACKS", "CANDIDATES", "COMBINATIONS"))
FIT_SCORE_MAX, FIT_WEIGHT_MAX = 1 << 40, 1024
# Per interval class 0..6 the weight of a common tick: the classes 1, 2 and 6 (seconds and sevenths, the tritone) are what
# evaluation.InterplayTotals calls dissonant and cost two, thirds, sixths, fourths and fifths earn one, unisons and octaves nothing.
# A stated convention, not a measured optimum
DEFAULT_FIT_WEIGHTS = (0, -2, -2, 1, 1, 1, -2)


class PairFit:
    """Device results of mhac_pair_fit on a candidate batch of S songs x T tracks x K candidates (row (s * T + t) * K + k, R = T * K
    rows a song): status int32 [B] (INTERPLAY_OK ...), ticks and pairs int64 [B, R, 7]: per row, per row of its song (local index
    t * K + k) and per interval class the common ticks (at most 65535 a pair) and the number of the note pairs that sound together;
    zeros for the row itself, the rows of its own track, rows out of range and every entry of a row that is not OK."""

    def __init__(self, status, ticks, pairs):
        self.status, self.ticks, self.pairs = status, ticks, pairs


class TrackChoice:
    """Device results of mhac_choose: choice int32 [S, T] (the kept candidate of every track; -1: a track without an eligible
    candidate), best and first int64 [S] (the objective of the choice, and of the smallest admissible combination: what one gets
    without choosing), status int32 [S] (CHOOSE_OK ...).  sampling.arrange adds rows int64 [S * T]: the chosen rows of the candidate
    batch (candidate 0 for a track that was left out)."""

    def __init__(self, choice, best, first, status):
        self.choice, self.best, self.first, self.status = choice, best, first, status


def _candidate_shape(what, S, T, K):
    S, T, K = int(S), int(T), int(K)
    if S < 1 or not 1 <= T <= CHOOSE_MAX_TRACKS or not 1 <= K <= CHOOSE_MAX_CANDIDATES:
        raise ValueError("%s: S >= 1, T in 1..%d and K in 1..%d (got %d, %d, %d)" % (what, CHOOSE_MAX_TRACKS, CHOOSE_MAX_CANDIDATES, S, T, K))
    return S, T, K


def pair_fit_raw(notes, counts3, meta, S, T, K, valid=None, shift=None):
    """mhac_pair_fit on the tensors a decode leaves: notes [B, max_notes, 4], counts3 [B, 3], meta [B, 11] with B = S * T * K rows in
    the candidate layout, valid [B] or None (every row), shift [B] ticks added to a row's notes or None -> PairFit.  The partners of
    a row are the rows of its song on another track; the rule is the header's.  ONE launch whatever the batch; nothing syncs with
    the host."""
    S, T, K = _candidate_shape("pair_fit", S, T, K)
    B, R = S * T * K, T * K
    if notes.dim() != 3 or notes.shape[2] != 4 or notes.shape[0] != B:
        raise ValueError("pair_fit: notes [S * T * K, max_notes, 4]")
    max_notes = notes.shape[1]
    if tuple(counts3.shape) != (B, 3) or tuple(meta.shape) != (B, 11):
        raise ValueError("pair_fit: counts [B, 3] and meta [B, 11]")
    if shift is not None and tuple(shift.shape) != (B,):
        raise ValueError("pair_fit: shift holds one entry per row")
    if not 1 <= max_notes <= INTERPLAY_MAX_NOTES or B * max_notes > 1 << 31:
        raise ValueError("pair_fit: max_notes in 1..%d and B * max_notes <= 2^31 (got %d, %d)" % (INTERPLAY_MAX_NOTES, max_notes, B))
    require_device(notes, counts3, meta, valid, shift)
    dev = notes.device
    notes, counts3, meta = (t.to(torch.int32).contiguous() for t in (notes, counts3, meta))
    valid = _mask_i32(valid, B, dev)
    shift = None if shift is None else shift.to(device=dev, dtype=torch.int32).contiguous()
    ticks = torch.empty(B, R, 7, device=dev, dtype=torch.int64)
    pairs = torch.empty(B, R, 7, device=dev, dtype=torch.int64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().mhac_pair_fit(ptr(notes), ptr(counts3), ptr(meta), ptr(valid), ptr(shift), ptr(ticks), ptr(pairs), ptr(status), S, T, K,
                              max_notes, current_stream()), "mhac_pair_fit")
    return PairFit(status, ticks, pairs)


def pair_fit(decoded, S, T, K, shift=None, valid=None):
    """pair_fit_raw on a DecodedBatch (utils.decode_util.decode_tokens) in the candidate layout; valid defaults to the rows that
    decoded (decoded.status == OK: the lists of the others hold nothing); shift: ticks per row, as
    utils.arrange_util.anchor_shift makes them."""
    if valid is None:
        valid = decoded.status == 0
    return pair_fit_raw(decoded.notes, decoded.counts, decoded.meta, S, T, K, valid, shift)


def fit_scores(ticks, weights=None):
    """ticks int64 [S * R, R, 7] (PairFit.ticks), weights: seven integers of magnitude <= 1024, one per interval class (default
    DEFAULT_FIT_WEIGHTS; a sequence, which is checked, or an int64 tensor, which is clamped to +-1024 where it lives) -> W int64 [S, R, R]: W[s, r, r'] = the sum over the
    classes of weights[class] * ticks[s * R + r, r', class], clamped to +-2^40.  A few torch operations where the ticks live (host
    tensors too); a pair of rows has at most 32768^2 pairs of at most 65535 ticks, so the int64 sum is exact."""
    if ticks.dim() != 3 or ticks.shape[2] != 7 or ticks.shape[1] < 1 or ticks.shape[0] % ticks.shape[1] or ticks.dtype != torch.int64:
        raise ValueError("fit_scores: ticks int64 [S * R, R, 7]")
    if isinstance(weights, torch.Tensor):
        w = weights.to(device=ticks.device, dtype=torch.int64)
        if tuple(w.shape) != (7,):
            raise ValueError("fit_scores: seven weights")
    else:
        host = [int(x) for x in (DEFAULT_FIT_WEIGHTS if weights is None else weights)]
        if len(host) != 7 or max(abs(x) for x in host) > FIT_WEIGHT_MAX:
            raise ValueError("fit_scores: seven integer weights of magnitude <= %d" % FIT_WEIGHT_MAX)
        w = torch.tensor(host, dtype=torch.int64, device=ticks.device)
    R = ticks.shape[1]
    return (ticks * w.clamp(-FIT_WEIGHT_MAX, FIT_WEIGHT_MAX)).sum(2).clamp(-FIT_SCORE_MAX, FIT_SCORE_MAX).view(ticks.shape[0] // R, R, R)


def choose_tracks(W, S, T, K, unary=None, eligible=None):
    """mhac_choose: W int64 [S, R, R] pair scores (fit_scores), unary int64 [S, R] or None (zeros), eligible [S, R] or None (every
    row) -> TrackChoice: per song the admissible combination of one candidate a track with the largest sum of unary and pair scores,
    the smallest combination index on a tie.  Exact enumeration: K^T <= 2^20 (the library refuses more).  ONE launch; nothing syncs
    with the host."""
    S, T, K = _candidate_shape("choose_tracks", S, T, K)
    R = T * K
    if tuple(W.shape) != (S, R, R) or W.dtype != torch.int64:
        raise ValueError("choose_tracks: W int64 [S, T * K, T * K]")
    for name, t in (("unary", unary), ("eligible", eligible)):
        if t is not None and tuple(t.shape) != (S, R):
            raise ValueError("choose_tracks: %s [S, T * K]" % name)
    require_device(W, unary, eligible)
    dev = W.device
    W = W.contiguous()
    unary = None if unary is None else unary.to(device=dev, dtype=torch.int64).contiguous()
    eligible = None if eligible is None else (eligible != 0).to(device=dev, dtype=torch.int32).contiguous()
    choice = torch.empty(S, T, device=dev, dtype=torch.int32)
    best = torch.empty(S, device=dev, dtype=torch.int64)
    first = torch.empty(S, device=dev, dtype=torch.int64)
    status = torch.empty(S, device=dev, dtype=torch.int32)
    check(lib().mhac_choose(ptr(W), ptr(unary), ptr(eligible), ptr(choice), ptr(best), ptr(first), ptr(status), S, T, K,
                            current_stream()), "mhac_choose")
    return TrackChoice(choice, best, first, status)
