"""The evaluation end of a sampling run (run/sample.py:155-163, :245-273, :306-317) on the device: the gate on valid rows, 1NNC over
[ground truth | generated], CP and CV of one batch (`evaluate_batch`), and the six running totals (`MetricTotals`).

The reference copies the batch to the host, compacts the valid rows with a boolean index and walks them in Python.  Here the per-row
decode status is a mask: the fused nearest-neighbour kernel (metric.nearest) and the controllability counters skip masked rows, so no
row is moved, nothing is read back per batch, and the number of launches does not depend on the batch size.  `MetricTotals.summary()`
is the one device -> host copy of a run.
Generation mode has no ground truth (the reference reports nothing there): `evaluate_generated` and `GenerationTotals`, additions, say
what needs none - diversity and duplicates from the pair statistics of the generated set (metric.pair_stats), novelty against a corpus
(metric.nearest), CP and CV - under the same rules: masks instead of compaction, one copy at the summary.
`HarmonyTotals`, an addition for every mode, is CH: how the decoded notes fit the chord progression the piece was conditioned on
(metric.harmony_counts), for the whole piece and, for an infill, inside and outside the regenerated bars.
`StructureTotals`, an addition for every mode, says whether the pieces are shaped like music over time (metric.structure_counts): the
pitch-class entropy of 1-bar and 4-bar windows and the groove similarity of the bars, read as a gap to real data (`structure_gap`).
`InterplayTotals`, an addition for runs whose rows are the tracks of songs (sampling.run_arrangement), says how the tracks of a song
fit each other (metric.interplay_counts): which intervals sound between them and for how long, and whether the bass lies below."""
import math

import torch

from . import metric
from .utils import decode_util as du

# statuses the reference reports as a SequenceToMidiError: the row is invalid and the run goes on (decode_util.write_decoded_rows)
_INVALID = (du.NO_EOS, du.RESTORE_FAILED, du.ONCE_FAILED, du.STRICT_FAILED)
_FATAL_EXC = {du.REF_INDEXERROR: IndexError, du.BAD_META: KeyError}


class BatchMetrics:
    """Device results of one batch.  valid [B] bool; valid_count int64 scalar; onnc fp32 scalar (NaN when no row is valid); counts
    int64 [4] = (CP total, CP wrong, CV total, CV wrong) over the valid rows; most int32 [2 B] (metric.ONNC_sets); fatal int32 scalar:
    0, or the largest decode status of the batch that makes write_decoded_rows raise (REF_INDEXERROR, BAD_META, OVERFLOW; a ground-truth
    row of a valid pair that does not split counts as its status too); decoded: the DecodedBatch the statuses came from."""

    def __init__(self, valid, valid_count, onnc, counts, most, fatal, decoded):
        self.valid, self.valid_count, self.onnc, self.counts, self.most, self.fatal, self.decoded = valid, valid_count, onnc, counts, most, fatal, decoded

    def vector(self):
        """fp64 [6] = (valid_count, onnc, CP total, CP wrong, CV total, CV wrong): what the per-batch report prints"""
        return torch.cat([self.valid_count.double().reshape(1), self.onnc.double().reshape(1), self.counts.double()])


def _fatal_of(status, where):
    bad = where & (status != du.OK)
    for st in _INVALID:
        bad = bad & (status != st)
    return torch.where(bad, status, torch.zeros_like(status)).max()


def evaluate_batch(sample_tokens, correct_ids, input_mask, strict_validation=True):
    """run/sample.py:245-273 for one batch of device tensors [B, L] -> BatchMetrics.  One decode_tokens gives the per-row status
    (valid = status OK; the driver writes its files from the same DecodedBatch), split_meta_midi(correct_ids) the ground-truth note rows,
    ONNC_sets and controllability_counts take the validity mask.  No .item(), no boolean-index compaction, no nonzero."""
    dec = du.decode_tokens(sample_tokens, input_mask, strict_validation)
    status = dec.status
    valid = status == du.OK
    gt, gt_len, _, gt_status = du.split_meta_midi(correct_ids, input_mask)
    every = torch.ones_like(valid)
    fatal = torch.maximum(_fatal_of(status, every), torch.where(valid, gt_status, torch.zeros_like(gt_status)).max())
    onnc, most = metric.ONNC_sets(gt, dec.restored, gt_len, dec.lengths, valid=valid, return_mostsim=True)
    counts = metric.controllability_counts(dec.meta, dec.restored, dec.lengths, valid=valid)
    return BatchMetrics(valid, valid.sum(), onnc, counts, most, fatal.to(torch.int32), dec)


class MetricTotals:
    """The accumulators of run/sample.py:157-163 as device scalars: onnc_sum fp32 as in the reference, onnc_count, total_total_p,
    total_total_v, total_wrong_p, total_wrong_v int64; `fatal` carries the BatchMetrics flags.
    The reference decodes rank after rank and broadcasts the totals from the rank that just decoded (run/sample.py:288-291).  That is
    not reproduced: with this project's sharding every rank holds the gathered tokens of the global batch, so every rank computes
    identical totals without a collective."""
    NAMES = ("onnc_sum", "onnc_count", "total_total_p", "total_total_v", "total_wrong_p", "total_wrong_v")

    def __init__(self, device="cuda"):
        self.onnc_sum = torch.zeros((), device=device, dtype=torch.float32)
        for name in self.NAMES[1:]:
            setattr(self, name, torch.zeros((), device=device, dtype=torch.int64))
        self.fatal = torch.zeros((), device=device, dtype=torch.int32)

    def update(self, m):
        """`if valid_count:` of run/sample.py:245 as a `where`: a batch without a valid row (onnc = 0 / 0) adds nothing."""
        some = m.valid_count > 0
        self.onnc_sum += torch.where(some, m.valid_count * m.onnc, torch.zeros_like(m.onnc))
        self.onnc_count += m.valid_count
        self.total_total_p += m.counts[0]
        self.total_wrong_p += m.counts[1]
        self.total_total_v += m.counts[2]
        self.total_wrong_v += m.counts[3]
        self.fatal = torch.maximum(self.fatal, m.fatal)
        return self

    def vector(self):
        """fp64 [7] on the device: the six totals in NAMES order, then the fatal status"""
        return torch.stack([getattr(self, n).double() for n in self.NAMES] + [self.fatal.double()])

    @staticmethod
    def raise_if_fatal(st):
        st = int(st)
        if st:
            raise _FATAL_EXC.get(st, RuntimeError)("%s (a row of the run; write_decoded_rows raises the same)" % du.STATUS_MESSAGE[st])

    @staticmethod
    def ratios(host):
        """host: the six totals as Python numbers -> the summary; a ratio with an empty denominator is NaN (the reference: tensor 0 / 0)"""
        div = lambda a, b: float(a) / float(b) if b else float("nan")
        return {"onnc": div(host[0], host[1]), "cp": div(host[4], host[2]), "cv": div(host[5], host[3]), "valid": float(host[1])}

    def summary(self):
        """{"onnc", "cp", "cv", "valid"} as Python floats (run/sample.py:309-311; valid = the rows counted): the one sync of a run.
        Raises what write_decoded_rows raises when a batch held a row of a fatal status."""
        host = self.vector().cpu().tolist()
        self.raise_if_fatal(host[6])
        return self.ratios(host)


def batch_block(batch_index, onnc, total_p, wrong_p, total_v, wrong_v):
    """run/sample.py:275-279"""
    div = lambda a, b: a / b if b else float("nan")
    return "\n".join([f"{f' Metric of Batch {batch_index} ':=^60}", f"{f' ONNC: {float(onnc):.6f} ': ^60}",
                      f"{f' CP: {div(wrong_p, total_p):.6f} ': ^60}", f"{f' CV: {div(wrong_v, total_v):.6f} ': ^60}", ("=" * 60) + "\n"])


def summary_block(s):
    """run/sample.py:312-317"""
    onnc, cp, cv = s["onnc"], s["cp"], s["cv"]
    return "\n".join(["", f"{f' Summary: Metric ':=^60}", f"{f' ONNC: {onnc:.6f} ': ^60}", f"{f' CP: {cp:.6f} ': ^60}",
                      f"{f' CV: {cv:.6f} ': ^60}", ("=" * 60) + "\n"])


# ------------------------------------------------------------------------------------------ generation mode: no ground truth (additions)
class GeneratedBatch:
    """Device results of one generated batch.  valid [B] bool; valid_count int64 scalar; vec fp32 [B, 56] (metric.get_vectors of the
    restored rows; the vector of an invalid row means nothing and is masked by `valid`); counts int64 [4] = (CP total, CP wrong,
    CV total, CV wrong) over the valid rows; fatal int32 scalar as in BatchMetrics; decoded: the DecodedBatch all of it came from."""

    def __init__(self, valid, valid_count, vec, counts, fatal, decoded):
        self.valid, self.valid_count, self.vec, self.counts, self.fatal, self.decoded = valid, valid_count, vec, counts, fatal, decoded


def evaluate_generated(sample_tokens, input_mask, strict_validation=False):
    """What a generated batch [B, L] says without a ground truth -> GeneratedBatch.  One decode_tokens gives the per-row status (valid =
    status OK; the driver writes its files from the same DecodedBatch); get_vectors runs on the restored rows and
    controllability_counts takes the validity mask.  No .item(), no compaction: the number of library launches does not depend on B."""
    dec = du.decode_tokens(sample_tokens, input_mask, strict_validation)
    valid = dec.status == du.OK
    fatal = _fatal_of(dec.status, torch.ones_like(valid))
    vec = metric.get_vectors(dec.restored, dec.lengths)
    counts = metric.controllability_counts(dec.meta, dec.restored, dec.lengths, valid=valid)
    return GeneratedBatch(valid, valid.sum(), vec, counts, fatal.to(torch.int32), dec)


class GenerationTotals:
    """What a generation run says about the set it made: are the pieces different from each other (diversity), how many are the same
    piece twice (duplicates), did the model copy a corpus (novelty, memorised), do they respect the ranges their meta asks for (CP, CV).
    `update` keeps every batch's vectors, validity mask and group ids on the device (56 floats a row) and adds the counts; `summary` is
    the one device -> host copy of a run: ONE metric.pair_stats call in self mode over all kept rows and, with a corpus [n, 56]
    (corpus_valid: its mask), ONE metric.nearest call against it.  With several ranks every rank holds the gathered tokens of the
    global batch and computes the same totals, as MetricTotals documents.
    duplicate_threshold: two rows are the same piece when their similarity reaches it.  The default is derived, not tuned: a unit-norm
    part of length n squared through an fmaf chain is within about (3 n + 6) 2^-24 of 1, which gives 188 * 2^-24 for the three parts
    and the two multiplies - below 256 * 2^-24 = 2^-16, so identical pieces always count as duplicates."""

    def __init__(self, device="cuda", duplicate_threshold=1 - 2.0 ** -16, corpus=None, corpus_valid=None):
        self.device, self.duplicate_threshold, self.corpus, self.corpus_valid = device, float(duplicate_threshold), corpus, corpus_valid
        self.vec, self.valid, self.groups = [], [], []
        self.counts = torch.zeros(4, device=device, dtype=torch.int64)
        self.valid_count = torch.zeros((), device=device, dtype=torch.int64)
        self.fatal = torch.zeros((), device=device, dtype=torch.int32)

    def update(self, m, groups=None):
        """m: a GeneratedBatch; groups: an integer id per row [B] (only rows of one group are compared; default: one group)"""
        self.vec.append(m.vec)
        self.valid.append(m.valid)
        self.groups.append(torch.zeros(m.vec.shape[0], device=m.vec.device, dtype=torch.int32) if groups is None
                           else groups.to(device=m.vec.device, dtype=torch.int32))
        self.counts += m.counts
        self.valid_count += m.valid_count
        self.fatal = torch.maximum(self.fatal, m.fatal)
        return self

    def vector(self):
        """fp64 [13] on the device: valid rows, sum of count, sum of nan, sum of sum, valid rows with a duplicate, CP total, CP wrong,
        CV total, CV wrong, fatal status, then with a corpus (else zeros) the sum and the number of the non-NaN best similarities and
        the valid rows whose best similarity reaches the threshold"""
        dev = self.valid_count.device
        zero = torch.zeros((), device=dev, dtype=torch.float64)
        pair, corp = [zero] * 4, [zero] * 3
        if self.vec:
            vec, valid = torch.cat(self.vec), torch.cat(self.valid)
            st = metric.pair_stats(vec, valid=valid, groups=torch.cat(self.groups), threshold=self.duplicate_threshold)
            pair = [st.count.sum(), st.nan.sum(), st.sum.sum(), (valid & (st.above > 0)).sum()]
            if self.corpus is not None:
                most, best = metric.nearest(vec, keys=self.corpus, valid=valid, keys_valid=self.corpus_valid, return_values=True)
                found = valid & (most >= 0) & ~torch.isnan(best)
                corp = [torch.where(found, best.double(), zero).sum(), found.sum(), (found & (best >= self.duplicate_threshold)).sum()]
        head = [self.valid_count] + pair + list(self.counts) + [self.fatal] + corp
        return torch.stack([x.double() for x in head])

    def ratios(self, host):
        """host: vector() as Python numbers -> the summary; a ratio with an empty denominator is NaN"""
        div = lambda a, b: float(a) / float(b) if b else float("nan")
        out = {"valid": int(host[0]), "pairs": int(host[1]) // 2, "nan_pairs": int(host[2]) // 2, "diversity": 1 - div(host[3], host[1]),
               "duplicates": div(host[4], host[0]), "cp": div(host[6], host[5]), "cv": div(host[8], host[7])}
        if self.corpus is not None:
            out.update(novelty=1 - div(host[10], host[11]), memorised=div(host[12], host[0]))
        return out

    def summary(self):
        """{"valid", "pairs", "nan_pairs", "diversity", "duplicates", "cp", "cv"[, "novelty", "memorised"]}: valid = the valid rows
        counted; pairs / nan_pairs = the unordered counted pairs whose similarity is a number / NaN; diversity = 1 - mean similarity
        over the counted pairs; duplicates = valid rows with a partner at or above the threshold / valid rows; cp, cv as in
        MetricTotals.summary(); with a corpus, novelty = 1 - mean of the non-NaN best similarities against it and memorised = the
        share of valid rows whose best similarity reaches the threshold.  The one sync of a run; raises what MetricTotals.summary()
        raises when a batch held a row of a fatal status."""
        host = self.vector().cpu().tolist()
        MetricTotals.raise_if_fatal(host[9])
        return self.ratios(host)


# ------------------------------------------------------------------------------------------ chord fit of a run (additions)
_first_bar_shift = du.first_bar_shift                    # shared with utils.arrange_util.align_shift


class HarmonyTotals:
    """The chord fit of a run as device integers: the seven sums of metric.harmony_counts (notes, judged, chord tones, scale tones and
    the three tick sums), the pitch-class histogram and, once `update` was given `bars`, (judged, chord tones) inside and outside that
    bar range.  One mhh_harmony_counts launch per `update` on the DecodedBatch the loop has anyway; `summary` is the one device -> host
    copy.  With several ranks every rank holds the gathered tokens and computes the same totals, as MetricTotals documents."""

    def __init__(self, device="cuda"):
        self.totals = torch.zeros(7, device=device, dtype=torch.int64)
        self.hist = torch.zeros(12, device=device, dtype=torch.int64)
        self.region = torch.zeros(2, device=device, dtype=torch.int64)
        self.rest = torch.zeros(2, device=device, dtype=torch.int64)
        self.rows = torch.zeros((), device=device, dtype=torch.int64)
        self.with_bars = False

    def update(self, decoded, valid=None, bars=None):
        """decoded: a DecodedBatch; valid: [B] mask (default: the rows that decoded); bars: (lo, hi) for every row or an int tensor
        [B, 2] in the bar ordinals of an infill plan (counted from the first BAR of the note region).  With bars the per-bar table
        says how the notes of bars lo <= k < hi fit (region) and the rest of the piece is the complement (rest)."""
        if bars is None:
            hc = metric.harmony_counts(decoded, valid, 0, return_hist=True)
        else:
            # large enough for the batch without asking the device: a bar needs a BAR token (the first may come without one)
            max_bars = min(metric.HARMONY_MAX_BARS, decoded.restored.shape[1] + 1)
            hc = metric.harmony_counts(decoded, valid, max_bars, return_hist=True)
            B, dev = hc.counts.shape[0], hc.counts.device
            if torch.is_tensor(bars):
                if tuple(bars.shape) != (B, 2):
                    raise ValueError("harmony: bars is (lo, hi) or an int tensor [B, 2], got %s" % (tuple(bars.shape),))
                lohi = bars.to(dev).long()
            else:
                lohi = torch.tensor([[int(bars[0]), int(bars[1])]], dtype=torch.int64, device=dev).expand(B, 2)
            lohi = lohi + _first_bar_shift(decoded).unsqueeze(1)
            k = torch.arange(max_bars, device=dev).unsqueeze(0)
            inside = ((k >= lohi[:, :1]) & (k < lohi[:, 1:])).unsqueeze(2)
            region = torch.where(inside, hc.bars[:, :, 1:3], torch.zeros_like(hc.bars[:, :, 1:3])).sum((0, 1), dtype=torch.int64)
            self.region += region
            self.rest += hc.counts[:, 1:3].sum(0, dtype=torch.int64) - region
            self.with_bars = True
        self.totals += hc.counts[:, :7].sum(0, dtype=torch.int64)
        self.hist += hc.hist.sum(0, dtype=torch.int64)
        self.rows += (hc.status == metric.HARMONY_OK).sum()
        return self

    def vector(self):
        """int64 [24] on the device: the seven sums, the histogram (12), region (2), rest (2), the rows counted"""
        return torch.cat([self.totals, self.hist, self.region, self.rest, self.rows.reshape(1)])

    def ratios(self, host):
        """host: vector() as Python ints -> the summary; a ratio with an empty denominator is NaN"""
        div = lambda a, b: float(a) / float(b) if b else float("nan")
        notes, judged, tones, in_scale, ticks, judged_ticks, tone_ticks = (int(x) for x in host[:7])
        hist = [int(x) for x in host[7:19]]
        total, entropy = sum(hist), float("nan")
        if total:
            entropy = 0.0
            for x in hist:
                if x:
                    p = float(x) / float(total)
                    entropy -= p * math.log2(p)
        out = {"rows": int(host[23]), "notes": notes, "judged": judged, "ch": div(judged - tones, judged),
               "ch_ticks": div(judged_ticks - tone_ticks, judged_ticks), "out_of_scale": div(notes - in_scale, notes),
               "judged_share": div(judged, notes), "pitch_class_entropy": entropy}
        if self.with_bars:
            region, rest = host[19:21], host[21:23]
            out.update(ch_region=div(region[0] - region[1], region[0]), ch_rest=div(rest[0] - rest[1], rest[0]),
                       judged_region=int(region[0]), judged_rest=int(rest[0]))
        return out

    def summary(self):
        """{"rows", "notes", "judged", "ch", "ch_ticks", "out_of_scale", "judged_share", "pitch_class_entropy"[, "ch_region", "ch_rest",
        "judged_region", "judged_rest"]}: rows = the rows counted; ch = judged notes off their chord / judged notes; ch_ticks the same
        by sounding ticks; out_of_scale = notes outside the key's scale / notes; judged_share = judged / notes; pitch_class_entropy in
        bits, computed here in float64 from the integer histogram; with bars, ch inside and outside the bar range and the judged notes
        of each.  The one device -> host copy."""
        return self.ratios(self.vector().cpu().tolist())


def harmony_block(s):
    """the chord-fit summary of a run, in the style of summary_block"""
    rows, judged, notes = s["rows"], s["judged"], s["notes"]
    lines = ["", f"{' Summary: Harmony ':=^60}", f"{f' Rows: {rows} ': ^60}", f"{f' Judged notes: {judged} of {notes} ': ^60}"]
    names = (("ch", "CH"), ("ch_ticks", "CH by ticks"), ("out_of_scale", "Out of scale"), ("judged_share", "Judged share"),
             ("pitch_class_entropy", "Pitch-class entropy"), ("ch_region", "CH region"), ("ch_rest", "CH rest"))
    lines += [f"{f' {label}: {s[key]:.6f} ': ^60}" for key, label in names if key in s]
    return "\n".join(lines + [("=" * 60) + "\n"])


# ------------------------------------------------------------------------------------------ structure of a run (additions)
class StructureTotals:
    """How the pieces of a run are shaped over time, as device sums of metric.structure_counts: the pitch-class entropy of 1-bar and
    4-bar windows (H1, H4 of the MusDr set), the groove similarity of the bars (GS: 1 - the mean share of sixteenth-note slots on which
    two bars of a piece disagree about an onset), notes, onsets and empty bars per bar, pitch use per piece.  The numbers are read as a
    gap to the same statistics of real data (structure_gap).  One mhm_structure_counts launch per `update` on the DecodedBatch the loop
    has anyway; `summary` is the one device -> host copy.  With several ranks every rank holds the gathered tokens and computes the
    same totals, as MetricTotals documents."""
    INT_NAMES = ("rows", "rows_with_notes", "notes", "skipped", "bars", "bars_with_notes", "pitch_classes", "distinct_pitches",
                 "pitch_range", "onsets", "windows_1", "windows_4")
    FLOAT_NAMES = ("h1_sum", "h4_sum", "gs_sum", "gs_rows")
    RATIO_NAMES = ("h1", "h4", "gs", "notes_per_bar", "empty_bars", "pitch_classes", "pitch_range", "distinct_pitches", "onsets_per_bar")

    def __init__(self, device="cuda"):
        self.ints = torch.zeros(len(self.INT_NAMES), device=device, dtype=torch.int64)
        self.floats = torch.zeros(len(self.FLOAT_NAMES), device=device, dtype=torch.float64)

    def update(self, decoded, valid=None):
        """decoded: a DecodedBatch; valid: [B] mask (default: the rows that decoded).  No sync with the host."""
        # large enough for the batch without asking the device: a bar needs a BAR token (the first may come without one)
        max_bars = min(metric.STRUCTURE_MAX_BARS, decoded.restored.shape[1] + 1)
        sc = metric.structure_counts(decoded, valid, max_bars)
        c = sc.counts.long()
        ok = sc.status == metric.STRUCTURE_OK
        some = ok & (c[:, 0] > 0)
        zero = torch.zeros_like(c[:, 0])
        per_row = torch.stack([ok.long(), some.long(), c[:, 0], c[:, 1], c[:, 2], c[:, 3], c[:, 4], c[:, 5],
                               torch.where(some, c[:, 7] - c[:, 6], zero), c[:, 8], c[:, 12], c[:, 13]], 1)
        self.ints += per_row.sum(0)
        paired = ok & (c[:, 9] > 0)
        slots = torch.where(paired, c[:, 11] * c[:, 9], torch.ones_like(zero)).double()
        gs = torch.where(paired, 1.0 - c[:, 10].double() / slots, torch.zeros_like(slots))
        self.floats += torch.stack([sc.entropy[:, 0].sum(), sc.entropy[:, 1].sum(), gs.sum(), paired.sum().double()])
        return self

    def vector(self):
        """float64 [16] on the device: the twelve integer sums in INT_NAMES order (exact below 2^53), then FLOAT_NAMES"""
        return torch.cat([self.ints.double(), self.floats])

    @staticmethod
    def ratios(host):
        """host: vector() as Python numbers -> the summary; a ratio with an empty denominator is NaN"""
        div = lambda a, b: float(a) / float(b) if b else float("nan")
        rows, some, notes, skipped, bars, with_notes, pcs, distinct, prange, onsets, w1, w4 = (int(x) for x in host[:12])
        h1, h4, gs, gs_rows = (float(x) for x in host[12:16])
        return {"rows": rows, "notes": notes, "skipped": skipped, "bars": bars, "h1": div(h1, w1), "h4": div(h4, w4), "gs": div(gs, gs_rows),
                "notes_per_bar": div(notes, with_notes), "empty_bars": 1 - div(with_notes, bars), "pitch_classes": div(pcs, some),
                "pitch_range": div(prange, some), "distinct_pitches": div(distinct, some), "onsets_per_bar": div(onsets, with_notes)}

    def summary(self):
        """{"rows", "notes", "skipped", "bars", "h1", "h4", "gs", "notes_per_bar", "empty_bars", "pitch_classes", "pitch_range",
        "distinct_pitches", "onsets_per_bar"}: rows = the rows counted; notes / skipped = the notes that went into the bars / that did
        not (a pitch outside 0..127, a start before 0 or behind the table); bars = the bars used, empty ones between notes included;
        h1, h4 = the mean pitch-class entropy in bits of the 1-bar / 4-bar windows that hold a note; gs = the mean over the rows with
        two bars and more of 1 - diff / (slots per bar * pairs); notes_per_bar, onsets_per_bar over the bars with notes; empty_bars =
        the share of used bars without a note; pitch_classes, pitch_range (highest - lowest), distinct_pitches = means over the rows
        with notes.  The one device -> host copy."""
        return self.ratios(self.vector().cpu().tolist())


def structure_gap(a, b):
    """the absolute differences of the ratio fields of two StructureTotals summaries (generated against real data); NaN where either
    side is"""
    return {k: abs(float(a[k]) - float(b[k])) for k in StructureTotals.RATIO_NAMES}


def structure_block(s, title="Structure"):
    """the structure summary of a run (or, without the counts, a structure_gap), in the style of harmony_block"""
    lines = ["", f"{f' Summary: {title} ':=^60}"]
    if "rows" in s:
        rows, notes, bars = s["rows"], s["notes"], s["bars"]
        lines += [f"{f' Rows: {rows} ': ^60}", f"{f' Notes: {notes} in {bars} bars ': ^60}"]
    names = (("h1", "H1"), ("h4", "H4"), ("gs", "GS"), ("notes_per_bar", "Notes per bar"), ("onsets_per_bar", "Onsets per bar"),
             ("empty_bars", "Empty bars"), ("pitch_classes", "Pitch classes"), ("distinct_pitches", "Distinct pitches"),
             ("pitch_range", "Pitch range"))
    lines += [f"{f' {label}: {s[key]:.6f} ': ^60}" for key, label in names if key in s]
    return "\n".join(lines + [("=" * 60) + "\n"])


def structure_report(generated, reference=None):
    """what a loop's report carries as `structure`: {"generated"[, "reference", "gap"]} from two summaries"""
    out = {"generated": generated}
    if reference is not None:
        out.update(reference=reference, gap=structure_gap(generated, reference))
    return out


# ------------------------------------------------------------------------------------------ interplay of a run (additions)
class InterplayTotals:
    """How the tracks of the songs of a run fit each other, as device int64 sums of metric.interplay_counts: per interval class and
    per "this row is below / above" the ticks and the pairs of notes that sound together between a row and the other rows of its
    song, once over all rows and once per track role (meta[9]: tokens 719..725 -> rows 0..6 = unknown, main melody, sub melody,
    accompaniment, bass, pad, riff; anything else -> row 7), the rows counted, their notes, the accompanied ones and the songs seen.
    One mha_interplay_counts launch per `update` on the DecodedBatch the loop has anyway; `summary` is the one device -> host copy."""
    ROLES = 8
    BASS_ROW, MELODY_ROW = 4, 1
    SCALAR_NAMES = ("rows", "notes", "accompanied", "songs")
    RATIO_NAMES = ("dissonance", "unison", "accompanied", "bass_above", "melody_below")

    def __init__(self, device="cuda"):
        self.ticks = torch.zeros(9, device=device, dtype=torch.int64)
        self.pairs = torch.zeros(9, device=device, dtype=torch.int64)
        self.role_ticks = torch.zeros(self.ROLES, 9, device=device, dtype=torch.int64)
        self.role_pairs = torch.zeros(self.ROLES, 9, device=device, dtype=torch.int64)
        self.scalars = torch.zeros(len(self.SCALAR_NAMES), device=device, dtype=torch.int64)

    def update(self, decoded, song, valid=None, shift=None, pitched_only=True):
        """decoded: a DecodedBatch; song [B]: the song of every row; valid, shift, pitched_only: metric.interplay_counts'.  A song is
        seen when one of its rows is counted (status OK).  No sync with the host."""
        ic = metric.interplay_counts(decoded, song, valid, shift, pitched_only)
        ok = ic.status == metric.INTERPLAY_OK                          # the rows that are not OK hold zeros
        role = decoded.meta[:, 9].long() - 719
        role = torch.where((role >= 0) & (role < self.ROLES - 1), role, torch.full_like(role, self.ROLES - 1))
        self.ticks += ic.ticks.sum(0)
        self.pairs += ic.pairs.sum(0)
        self.role_ticks.index_add_(0, role, ic.ticks)
        self.role_pairs.index_add_(0, role, ic.pairs)
        song = torch.as_tensor(song).to(ok.device)
        b = torch.arange(len(ok), device=ok.device)
        earlier = ((song.unsqueeze(1) == song.unsqueeze(0)) & ok.unsqueeze(0) & (b.unsqueeze(0) < b.unsqueeze(1))).any(1)
        c = ic.counts.long()
        self.scalars += torch.stack([ok.sum(), c[:, 0].sum(), c[:, 3].sum(), (ok & ~earlier).sum()])
        return self

    def vector(self):
        """int64 [166] on the device: ticks (9), pairs (9), ticks per role (8 x 9), pairs per role (8 x 9), SCALAR_NAMES"""
        return torch.cat([self.ticks, self.pairs, self.role_ticks.reshape(-1), self.role_pairs.reshape(-1), self.scalars])

    @classmethod
    def ratios(cls, host):
        """host: vector() as Python ints -> the summary, computed in float64; a ratio with an empty denominator is NaN"""
        div = lambda a, b: float(a) / float(b) if b else float("nan")
        host = [int(x) for x in host]
        ticks, pairs = host[:9], host[9:18]
        role_ticks = [host[18 + 9 * r:27 + 9 * r] for r in range(cls.ROLES)]
        rows, notes, accompanied, songs = host[18 + 18 * cls.ROLES:]
        sounding = sum(ticks[:7])
        bass, melody = role_ticks[cls.BASS_ROW], role_ticks[cls.MELODY_ROW]
        return {"rows": rows, "songs": songs, "notes": notes, "pairs": sum(pairs[:7]) // 2, "ticks": sounding // 2,
                "dissonance": div(ticks[1] + ticks[2] + ticks[6], sounding), "unison": div(ticks[0], sounding),
                "accompanied": div(accompanied, notes), "bass_above": div(bass[8], bass[7] + bass[8]),
                "melody_below": div(melody[7], melody[7] + melody[8])}

    def summary(self):
        """{"rows", "songs", "notes", "pairs", "ticks", "dissonance", "unison", "accompanied", "bass_above", "melody_below"}: rows =
        the rows counted, songs = the songs with a counted row, notes = their counted notes; pairs / ticks = the unordered pairs of
        notes of two tracks of a song that sound together and their common ticks (every pair is seen from both rows); dissonance =
        the ticks of interval classes 1, 2 and 6 (seconds, sevenths, the tritone) over the ticks of all seven; unison = the ticks of
        class 0 (unisons, octaves) over the same sum; accompanied = the share of counted notes that sound together with a note of
        another track; bass_above = of the ticks the bass rows share with a note of another pitch, those where the bass is the
        higher; melody_below = the same for the main-melody rows and the lower.  The one device -> host copy."""
        return self.ratios(self.vector().cpu().tolist())


def interplay_block(s):
    """the interplay summary of a run, in the style of harmony_block"""
    rows, songs, pairs, notes = s["rows"], s["songs"], s["pairs"], s["notes"]
    lines = ["", f"{' Summary: Interplay ':=^60}", f"{f' Songs: {songs} ({rows} tracks, {notes} notes) ': ^60}",
             f"{f' Pairs sounding together: {pairs} ': ^60}"]
    names = (("dissonance", "Dissonance"), ("unison", "Unison"), ("accompanied", "Accompanied"), ("bass_above", "Bass above"),
             ("melody_below", "Melody below"))
    lines += [f"{f' {label}: {s[key]:.6f} ': ^60}" for key, label in names]
    return "\n".join(lines + [("=" * 60) + "\n"])


def generation_block(s):
    """the summary of a generation run, in the style of summary_block"""
    valid, pairs = s["valid"], s["pairs"]
    lines = ["", f"{' Summary: Generation ':=^60}", f"{f' Valid: {valid} ': ^60}", f"{f' Pairs: {pairs} ': ^60}"]
    names = (("diversity", "Diversity"), ("duplicates", "Duplicates"), ("cp", "CP"), ("cv", "CV"), ("novelty", "Novelty"), ("memorised", "Memorised"))
    lines += [f"{f' {label}: {s[key]:.6f} ': ^60}" for key, label in names if key in s]
    return "\n".join(lines + [("=" * 60) + "\n"])
