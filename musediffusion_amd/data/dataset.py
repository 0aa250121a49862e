"""MuseDiffusion/data/__init__.py:14-89 load_data_music with the dataset resident on the device.

    MusicDataset       the ComMU `input_*.npy` / `target_*.npy` pair, merged once by mh_merge_and_mask (helper_tokenize, data/preprocess.py:26-70)
                       and filtered by length (helper_filter, :73-81 under the rule of :116); ragged input_ids / input_mask on the device
    augment_rows       commu/preprocessor/augment.py's key and tempo augmentation as a token map on merged rows (csrc/loader.hip)
    MusicLoader        wrap_dataset's DataLoader (data/wrapper.py:10-39): torch's own epoch order on the host, the batch on the device -
                       gather, augment, per-sequence corruption (wrapper.py:73-87), collate_batches
    load_data_music    the reference's arguments with their meaning

Not reproduced: tokenize_with_caching's Arrow cache and its lock file (preprocess.py:84-147) - the merge runs on the device in
milliseconds, so there is nothing worth caching; nothing is downloaded either (download.py): a missing file is an error."""
import itertools
import os

import numpy as np
import torch

from .._lib import ABI, check, current_stream, lib, ptr, require_device
from .corruption import Corruptions
from .wrapper import _pad, collate_batches, gather_rows, to_ragged

# enum mhd_augment_status (include/musehip_data.h)
AUGMENT_OK, NOT_ORIGIN, PITCH_RANGE, BAD_ROW = (ABI["musehip_data.h"].enums["MHD_AUGMENT_" + n] for n in ("OK", "NOT_ORIGIN", "PITCH_RANGE", "BAD_ROW"))
# commu/preprocessor/utils/constants.py:28-29 and augment.py:94-97: key_change in range(-6, 6), bpm_change in range(-2, 3)
KEY_CHANGES, BPM_CHANGES = range(-6, 6), range(-2, 3)
FILTER_BELOW = 2096                    # preprocess.py:116: rows are filtered by length only when seq_len < 2096
MERGE_CHUNK = 1024                     # rows per mh_merge_and_mask call


def augment_rows(values, offsets, key_change=None, bpm_change=None, return_status=False):
    """The 12 key changes x 5 tempo changes the reference writes as MIDI files before encoding (augment.py:88-98), applied to merged
    rows on the fly: key_change[b] in -6..5, bpm_change[b] in -2..2 (int, [B]; default: drawn uniformly over that grid from torch's
    device generator).  The tempo token (index 0) moves by bpm_change bins, the key token (index 1) and every pitch and chord-root token
    from index 11 on by key_change semitones; the pitch-range token is left as it is (the reference copies the parent's meta).
    status [B]: AUGMENT_OK, or NOT_ORIGIN (key token not cmajor / aminor), PITCH_RANGE (a pitch would leave 0..127), BAD_ROW (fewer
    than 12 tokens, more than the row limit, a draw off the grid) - such rows come back unchanged, as the reference makes no variant."""
    require_device(values, offsets)
    values, offsets = values.to(torch.int32).contiguous(), offsets.to(torch.int64).contiguous()
    B, dev = offsets.numel() - 1, values.device
    if key_change is None:
        key_change = torch.randint(KEY_CHANGES.start, KEY_CHANGES.stop, (B,), device=dev, dtype=torch.int32)
    if bpm_change is None:
        bpm_change = torch.randint(BPM_CHANGES.start, BPM_CHANGES.stop, (B,), device=dev, dtype=torch.int32)
    key_change = torch.as_tensor(key_change).to(device=dev, dtype=torch.int32).contiguous()
    bpm_change = torch.as_tensor(bpm_change).to(device=dev, dtype=torch.int32).contiguous()
    assert key_change.shape == (B,) and bpm_change.shape == (B,)
    out = torch.empty_like(values)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().mhd_augment_rows(ptr(values), ptr(offsets), ptr(key_change), ptr(bpm_change), ptr(out), ptr(status), B, current_stream()),
          "mhd_augment_rows")
    return (out, status) if return_status else out


class Augment:
    """augment_rows as the loader's batch stage: `Augment()(values, offsets)` draws one (key, tempo) change per row"""

    def __call__(self, values, offsets):
        return augment_rows(values, offsets)

    def __repr__(self):
        return "Augment(key_change=%d..%d, bpm_change=%d..%d)" % (KEY_CHANGES[0], KEY_CHANGES[-1], BPM_CHANGES[0], BPM_CHANGES[-1])


def _load_pair(data_dir, split):
    """load_raw_data (preprocess.py:8-23): 'train' reads input_train / target_train, 'valid' and 'test' read input_val / target_val"""
    split = str(split).lower()
    assert split in ("train", "valid", "test"), "invalid split for dataset"
    tag = "train" if split == "train" else "val"
    pair = []
    for kind in ("input", "target"):
        path = os.path.join(str(data_dir), "%s_%s.npy" % (kind, tag))
        if not os.path.isfile(path):
            raise FileNotFoundError("ComMU dataset file %s not found (nothing is downloaded: put input_%s.npy and target_%s.npy into %s)"
                                    % (path, tag, tag, data_dir))
        pair.append(np.load(path, allow_pickle=True))
    return pair


class MusicDataset:
    """The merged dataset on the device: `fields` = {'input_ids', 'input_mask'} ragged int32 values sharing `offsets` (int64 [n + 1]),
    and `lengths` - the n row lengths as a host numpy array, from which the width of a bucketed batch is known without a sync."""

    def __init__(self, fields, offsets, lengths, seq_len):
        self.fields, self.offsets, self.lengths, self.seq_len = fields, offsets, np.asarray(lengths, np.int64), seq_len
        self.max_len = int(self.lengths.max()) if len(self.lengths) else 0

    def __len__(self):
        return len(self.lengths)

    @property
    def device(self):
        return self.offsets.device

    @classmethod
    def from_dir(cls, data_dir, split, seq_len, device="cuda"):
        src, trg = _load_pair(data_dir, split)
        return cls.from_rows(list(src), list(trg), seq_len, device)

    @classmethod
    def from_rows(cls, src_rows, trg_rows, seq_len, device="cuda"):
        """src_rows[i]: the meta tokens of row i, trg_rows[i]: its event words.  Both go to the device once, are merged in chunks of
        MERGE_CHUNK rows (the words padded to the chunk's longest row) and, when seq_len < 2096, lose the rows longer than seq_len."""
        from ..utils.encode_util import OK, merge_and_mask
        assert len(src_rows) == len(trg_rows)
        seq_len = FILTER_BELOW if seq_len is None else int(seq_len)      # no seq_len (bucketing only): nothing is filtered
        max_row = int(lib().mh_batch_max_row())
        src_rows = [np.asarray(r, np.int64).reshape(-1) for r in src_rows]
        trg_rows = [np.asarray(r, np.int64).reshape(-1) for r in trg_rows]
        src_len = np.array([len(r) for r in src_rows], np.int64)
        trg_len = np.array([len(r) for r in trg_rows], np.int64)
        filtering = seq_len < FILTER_BELOW
        fits = (src_len <= max_row) & (trg_len <= max_row)
        if not fits.all() and not (filtering and seq_len <= max_row):    # a row that long is longer than seq_len once merged
            raise ValueError("a row of more than %d tokens: the merge kernel cannot hold it" % max_row)
        sv, so = to_ragged(src_rows, device)
        tv, to = to_ragged(trg_rows, device)
        require_device(sv, tv)
        ids, masks, lens = [], [], []
        for lo in range(0, len(src_rows), MERGE_CHUNK):
            hi = min(lo + MERGE_CHUNK, len(src_rows))
            S = int(min(max(src_len[lo:hi].max(), 1), max_row))
            ld = int(min(max(trg_len[lo:hi].max(), 1), max_row))
            src = _pad(sv, so[lo:hi + 1], S, 0)
            words = _pad(tv, to[lo:hi + 1], ld, 0)
            n_src = torch.from_numpy(np.minimum(src_len[lo:hi], S).astype(np.int32)).to(device)
            n_trg = torch.from_numpy(np.minimum(trg_len[lo:hi], ld).astype(np.int32)).to(device)
            fields, offsets, length, status = merge_and_mask(src, words, n_trg, src_len=n_src)
            length_h = length.cpu().numpy().astype(np.int64)             # the one sync per chunk, at load time
            assert not status.cpu().numpy().any() and OK == 0
            keep = fits[lo:hi] & ((length_h <= seq_len) if filtering else True)
            kept = np.nonzero(keep)[0]
            if len(kept) == 0:
                continue
            total = int(length_h[kept].sum())
            got, _, _ = gather_rows(fields, offsets, torch.from_numpy(kept).to(device), total)
            ids.append(got["input_ids"][:total])
            masks.append(got["input_mask"][:total])
            lens.append(length_h[kept])
        lens = np.concatenate(lens) if lens else np.zeros(0, np.int64)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(device)
        cat = lambda parts: torch.cat(parts) if parts else torch.zeros(0, device=device, dtype=torch.int32)
        return cls({"input_ids": cat(ids), "input_mask": cat(masks)}, offsets, lens, seq_len)


class MusicLoader:
    """wrap_dataset's DataLoader (wrapper.py:31-38) over a MusicDataset.  `iter(loader)` is one epoch, `len(loader)` its number of
    batches (the last partial batch is kept).  The order of rows is torch.utils.data.DataLoader's: iter() draws the DataLoader's
    base seed from torch's default generator, and with shuffle the first batch draws RandomSampler's seed for a fresh torch.randperm -
    so under the same torch.manual_seed the batches hold the rows a DataLoader(shuffle=...) over the same dataset would."""

    def __init__(self, dataset, batch_size, shuffle, corruption=None, use_bucketing=True, seq_len=None, augment=None):
        assert batch_size >= 1 and (use_bucketing or seq_len)
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.corruption, self.augment, self.use_bucketing, self.seq_len = corruption, augment, bool(use_bucketing), seq_len

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def index_batches(self):
        """the row indices of one epoch, batch by batch (host only)"""
        torch.empty((), dtype=torch.int64).random_()                      # _BaseDataLoaderIter.__init__: _base_seed
        return self._index_batches()

    def _index_batches(self):
        n = len(self.dataset)
        if self.shuffle:                                                  # RandomSampler.__iter__ without a generator of its own
            g = torch.Generator()
            g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            order = torch.randperm(n, generator=g)
        else:
            order = torch.arange(n)
        for lo in range(0, n, self.batch_size):
            yield order[lo:lo + self.batch_size]

    def batch(self, idx):
        """rows idx (int64 host tensor) -> the dict of collate_batches, on the device"""
        ds = self.dataset
        lens = ds.lengths[idx.numpy()]                                    # host: the batch's token count and width need no sync
        fields, offsets, _ = gather_rows(ds.fields, ds.offsets, idx.to(ds.device, non_blocking=True), int(lens.sum()))
        ids = fields["input_ids"]
        if self.augment is not None:
            ids = self.augment(ids, offsets)
        out = {"input_mask": fields["input_mask"]}
        if self.corruption is not None:
            out["correct_ids"] = ids
            ids = self.corruption(ids, offsets, per_sequence=True)
        out["input_ids"] = ids
        width = int(lens.max()) if self.use_bucketing else int(self.seq_len)
        return collate_batches(out, offsets, width)

    def __iter__(self):
        return (self.batch(idx) for idx in self.index_batches())


def _infinite(loader):
    """infinite_loader_from_iterable (wrapper.py:134-136)"""
    while True:
        yield from loader


def load_data_music(split="train", batch_size=1, data_dir=None, use_corruption=False, corr_available=None, corr_max=None, corr_p=None,
                    corr_kwargs=None, use_bucketing=True, seq_len=None, deterministic=False, loop=True, num_preprocess_proc=1,
                    num_loader_proc=0, *, augment=False, device="cuda"):
    """The reference's load_data_music (data/__init__.py:14-89) with its arguments: `split` 'train' / 'valid' / 'test' (a list or
    tuple gives a list of loaders), the corruption configuration, `use_bucketing` (pad to the longest row of the batch instead of
    seq_len), `deterministic` (no shuffling).  loop=True: an infinite iterator, its first batch already made; loop=False: an
    iterable giving one pass per iter(); loop=None: the MusicLoader itself.  num_preprocess_proc and num_loader_proc are accepted and
    ignored - there are no worker processes.  Ours: `augment` switches the key / tempo augmentation on (augment_rows), `device`.
    Every item is collate_batches' dict: 'input_ids', 'input_mask', 'length' and, under corruption, 'correct_ids' - int32, on the
    device: what TrainLoop, a TrainStep and sampling.modify take."""
    if isinstance(split, (list, tuple)):
        return [load_data_music(sp, batch_size, data_dir, use_corruption, corr_available, corr_max, corr_p, corr_kwargs, use_bucketing,
                                seq_len, deterministic, loop, num_preprocess_proc, num_loader_proc, augment=augment, device=device)
                for sp in split]
    if data_dir is None:
        raise FileNotFoundError("load_data_music: data_dir is not given (nothing is downloaded: name the directory of the ComMU "
                                "input_*.npy / target_*.npy files)")
    corruption = Corruptions.from_config(corr_available, corr_max, corr_p, corr_kwargs) if use_corruption else None
    dataset = MusicDataset.from_dir(data_dir, split, seq_len, device)
    loader = MusicLoader(dataset, batch_size, shuffle=not deterministic, corruption=corruption, use_bucketing=use_bucketing,
                         seq_len=seq_len, augment=Augment() if augment else None)
    if loop:
        it = _infinite(loader)
        return itertools.chain([next(it)], it)                            # __init__.py:85-87: the first batch is made here
    return loader
