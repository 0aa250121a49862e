"""Numpy restatement of the dataset loader (csrc/loader.hip, musediffusion_amd/data/dataset.py): ragged gather, row select, key / tempo
augmentation, the reference's per-sequence corruption over oracle.batch's corruption functions, and torch's DataLoader epoch order.
Pinned against the reference's recorded answers (tests/golden/loader.npz) by tests/test_loader_cpu.py; the GPU tests compare the
kernels with it bit for bit.  Test infrastructure only."""
import numpy as np
import torch

from oracle import batch as ob

GATHER_OK, BAD_INDEX, OVERFLOW = 0, 1, 2
AUGMENT_OK, NOT_ORIGIN, PITCH_RANGE, BAD_ROW = 0, 1, 2, 3
MAX_ROW = 4096
KEY_CHANGES, BPM_CHANGES = range(-6, 6), range(-2, 3)


def rows_of(values, offsets):
    return [np.asarray(values[offsets[b]:offsets[b + 1]]) for b in range(len(offsets) - 1)]


def ragged(rows, dtype=np.int32):
    rows = [np.asarray(r, dtype).reshape(-1) for r in rows]
    lens = [len(r) for r in rows]
    return (np.concatenate(rows).astype(dtype) if rows else np.zeros(0, dtype)), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ gather / select
def gather_offsets(src_offsets, idx, cap):
    """-> (out_offsets [B + 1], length [B], status [B]).  An index outside [0, n) is an empty row with BAD_INDEX.  The running sum stops
    at the first row whose end passes cap: that row and every later non-empty one become empty with OVERFLOW."""
    n, B = len(src_offsets) - 1, len(idx)
    length, status, offsets = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B + 1, np.int64)
    total, fit = 0, 0
    for b, i in enumerate(idx):
        ok = 0 <= i < n
        ln = int(src_offsets[i + 1] - src_offsets[i]) if ok else 0
        total += ln
        if total <= cap:
            fit, length[b] = total, ln
        status[b] = BAD_INDEX if not ok else OVERFLOW if (total > cap and ln > 0) else GATHER_OK
        offsets[b + 1] = fit
    return offsets, length, status


def gather_rows(src_values, src_offsets, idx, out_offsets, length, out):
    """writes the rows into `out` (a sentinel-filled array of cap tokens) in place, as the kernel does"""
    for b, i in enumerate(idx):
        if length[b] > 0:
            out[out_offsets[b]:out_offsets[b] + length[b]] = src_values[src_offsets[i]:src_offsets[i] + length[b]]
    return out


def select_rows(a, b, offsets, take_b):
    out = np.array(a, copy=True)
    for r in range(len(offsets) - 1):
        if take_b[r]:
            out[offsets[r]:offsets[r + 1]] = b[offsets[r]:offsets[r + 1]]
    return out


# ------------------------------------------------------------------------------------------------------------------ augmentation
def tempo_token(tok, c):
    """commu encoder/meta.py:119-123 encode_bpm of bpm + 5 c, on the token: 560 + m -> 560 + min(max(m + c, 1), 40); the clamp at 40 is
    MAX_BPM's, the clamp at 1 is ours (the reference has no tempo below 5)"""
    return 560 + min(max(tok - 560 + c, 1), 40) if 561 <= tok <= 600 else tok


def key_token(tok, k):
    """augment.py:40-56: MAJOR_KEY[origin + k] / MINOR_KEY[origin - 12 + k] with Python's negative indices and the IndexError branch,
    i.e. the key number moves by k modulo 12 inside its mode"""
    for base in (602, 614):
        if base <= tok < base + 12:
            return base + (tok - base + k) % 12
    return tok


def chord_token(tok, k):
    """utils/utils.py:37-96 sync_key_augment, then the encoder's vocabulary, where a flat root is an alias of the sharp one: the root
    index (a = 0) moves by k modulo 12, the quality stays; 303 (Chord_NN) has no root"""
    if 195 <= tok < 303:
        r, q = divmod(tok - 195, 9)
        return 195 + 9 * ((r + k) % 12) + q
    return tok


def augment_row(row, k, c):
    """-> (row, status).  NOT_ORIGIN is decided before PITCH_RANGE; in every non-OK case the row comes back unchanged."""
    row = np.asarray(row, np.int32)
    if len(row) < 12 or len(row) > MAX_ROW or k not in KEY_CHANGES or c not in BPM_CHANGES:
        return row.copy(), BAD_ROW
    if row[1] not in (602, 623):                                          # preprocessor.py:231-234: cmajor / aminor only
        return row.copy(), NOT_ORIGIN
    body = row[11:]
    pitch = (body >= 3) & (body <= 130)
    if ((body[pitch] + k < 3) | (body[pitch] + k > 130)).any():           # augment.py:64-69: dump raises, the file is dropped
        return row.copy(), PITCH_RANGE
    out = row.copy()
    out[0], out[1] = tempo_token(int(row[0]), c), key_token(int(row[1]), k)
    out[11:] = [t + k if 3 <= t <= 130 else chord_token(int(t), k) for t in body]
    return out, AUGMENT_OK


def augment_rows(values, offsets, key_change, bpm_change):
    res = [augment_row(r, int(k), int(c)) for r, k, c in zip(rows_of(values, offsets), key_change, bpm_change)]
    return (np.concatenate([r for r, _ in res]) if res else np.zeros(0, np.int32)), np.array([s for _, s in res], np.int32)


# ------------------------------------------------------------------------------------------------------------------ corruption
def corrupt_per_sequence(values, offsets, choices, available, draws, p=None, count=3):
    """MuseDiffusion/data/corruption.py:47-56 per row: slot r applies corruption available[choices[b, r]] (none for -1) to row b.
    draws: dict with 'u' [slots, tokens], 'new' [slots, tokens, 3], 'pairs' [slots, B, count, 2], indexed per row as the kernels take
    them (u / new at offsets[b] + draw number)."""
    p = dict(mt=0.3, mn=0.5, rn=0.5, **(p or {}))
    out = []
    for b, row in enumerate(rows_of(values, offsets)):
        row = row.astype(np.int32)
        lo, hi = offsets[b], offsets[b + 1]
        for r in range(choices.shape[1]):
            if choices[b, r] < 0:
                continue
            key = available[choices[b, r]]
            u = draws["u"][r, lo:hi].astype(np.float32)
            if key == "mt":
                row = ob.masking_token(row, u, np.float32(p["mt"]))
            elif key == "mn":
                row = ob.masking_note(row, u, np.float32(p["mn"]))
            elif key == "rn":
                row = ob.randomize_note(row, u, draws["new"][r, lo:hi], np.float32(p["rn"]))
            else:
                row = ob.random_rotating(row, draws["pairs"][r, b][:count])
        out.append(row)
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------------------------ epoch order
def epoch_batches(n, batch_size, shuffle):
    """the index batches of one pass of torch.utils.data.DataLoader(range(n), batch_size, shuffle) from torch's default generator:
    the iterator draws its base seed, then RandomSampler (shuffle only) a seed for the generator of one torch.randperm(n)"""
    torch.empty((), dtype=torch.int64).random_()
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    return [order[lo:lo + batch_size] for lo in range(0, n, batch_size)]


def rotate_name(name, k):
    """a chord name with its root moved by k semitones, the black keys spelled flat as sync_key_augment's symbol2chord spells them
    (the vocabulary knows the abstract qualities on natural and flat roots only)"""
    sharp = ("a", "a#", "b", "c", "c#", "d", "d#", "e", "f", "f#", "g", "g#")
    flat = ("a", "bb", "b", "c", "db", "d", "eb", "e", "f", "gb", "g", "ab")
    low = name.lower()
    root = low[:2] if low[1:2] == "#" or low[:2] in flat else low[:1]
    at = sharp.index(root) if root in sharp else flat.index(root)
    return flat[(at + k) % 12] + low[len(root):]
