"""collate_batches of MuseDiffusion/data/wrapper.py:90-127 on the device: ragged fields -> padded [B, seq_len] tensors; and the two
ragged tools of the dataset loader (data/dataset.py): gather rows by index, select rows between two buffers."""
import torch

from .._lib import check, current_stream, lib, ptr, require_device


def to_ragged(rows, device):
    """list of 1-D int sequences -> (values int32 [sum len], offsets int64 [B + 1]) on `device` (one H2D copy each)"""
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    offsets = torch.zeros(len(rows) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(lens, 0)
    values = torch.cat([torch.as_tensor(r, dtype=torch.int32).reshape(-1) for r in rows]) if rows else torch.zeros(0, dtype=torch.int32)
    return values.to(device), offsets.to(device)


def gather_rows(fields, src_offsets, idx, cap, return_status=False):
    """rows idx[b] of a ragged source -> a ragged batch (csrc/loader.hip).  fields: dict name -> int32 values sharing `src_offsets`
    (int64 [n + 1]); idx int64 [B] on the device; cap: tokens each output field has room for (B x the longest source row always
    fits, and sizing it so needs no sync).  Returns ({name: values [cap]}, offsets int64 [B + 1], length int32 [B]) and, on request,
    status [B]: 1 = index outside [0, n), 2 = the row did not fit cap; such rows are empty.  Two + len(fields) launches."""
    require_device(src_offsets, idx)
    dev = src_offsets.device
    idx = idx.to(device=dev, dtype=torch.int64).contiguous()
    src_offsets = src_offsets.to(torch.int64).contiguous()
    B, n, cap = idx.numel(), src_offsets.numel() - 1, int(cap)
    offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    length, status = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().mhd_gather_offsets(ptr(src_offsets), n, ptr(idx), ptr(offsets), ptr(length), ptr(status), B, cap, current_stream()),
          "mhd_gather_offsets")
    out = {}
    for name, vals in fields.items():
        require_device(vals)
        vals = vals.to(torch.int32).contiguous()
        out[name] = torch.empty(max(cap, 1), device=dev, dtype=torch.int32)
        check(lib().mhd_gather_rows(ptr(vals), ptr(src_offsets), n, ptr(idx), ptr(offsets), ptr(length), ptr(out[name]), B, cap,
                                    current_stream()), "mhd_gather_rows")
    return (out, offsets, length, status) if return_status else (out, offsets, length)


def select_rows(a_values, b_values, offsets, take_b, out=None):
    """out row b = take_b[b] ? row b of b_values : row b of a_values, for ragged buffers sharing `offsets`; out may be a_values"""
    require_device(a_values, b_values, offsets, take_b)
    assert a_values.dtype == b_values.dtype == torch.int32 and a_values.is_contiguous() and b_values.is_contiguous()
    take_b = take_b.to(torch.int32).contiguous()
    offsets = offsets.to(torch.int64).contiguous()
    out = torch.empty_like(a_values) if out is None else out
    check(lib().mhd_select_rows(ptr(a_values), ptr(b_values), ptr(offsets), ptr(take_b), ptr(out), offsets.numel() - 1, current_stream()),
          "mhd_select_rows")
    return out


def _pad(values, offsets, L, pad, want_length=False):
    require_device(values, offsets)
    B = offsets.numel() - 1
    out = torch.empty(B, L, device=values.device, dtype=torch.int32)
    length = torch.empty(B, device=values.device, dtype=torch.int32) if want_length else None
    check(lib().mh_ragged_to_padded(ptr(values.to(torch.int32).contiguous()), ptr(offsets.to(torch.int64).contiguous()), ptr(out),
                                    ptr(length), B, L, int(pad), current_stream()), "mh_ragged_to_padded")
    return (out, length) if want_length else out


def collate_batches(fields, offsets, seq_len=None):
    """fields: dict name -> ragged int32 values sharing `offsets` (keys as in the reference: 'input_ids', 'input_mask',
    optional 'correct_ids', 'label').  Returns the reference's dict: ids / correct_ids / label zero padded, input_mask
    padded with ONES, plus 'length' (wrapper.py:100-127).  seq_len None = the longest row (one host sync to read it).
    Unlike the reference, which raises on a row longer than seq_len, such a row is truncated to its first seq_len tokens and
    'length' still reports its full length (so length[b] > seq_len marks it); an empty row is all padding with length 0."""
    L = int(seq_len) if seq_len else int((offsets[1:] - offsets[:-1]).max())
    out = {}
    for name, vals in fields.items():
        if name == "input_ids":
            out[name], out["length"] = _pad(vals, offsets, L, 0, want_length=True)
        else:
            out[name] = _pad(vals, offsets, L, 1 if name == "input_mask" else 0)
    return out
