"""The evaluation end of a sampling run (run/sample.py:155-163, :245-273, :306-317) on the device: the gate on valid rows, 1NNC over
[ground truth | generated], CP and CV of one batch (`evaluate_batch`), and the six running totals (`MetricTotals`).

The reference copies the batch to the host, compacts the valid rows with a boolean index and walks them in Python.  Here the per-row
decode status is a mask: the fused nearest-neighbour kernel (metric.nearest) and the controllability counters skip masked rows, so no
row is moved, nothing is read back per batch, and the number of launches does not depend on the batch size.  `MetricTotals.summary()`
is the one device -> host copy of a run."""
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
