"""Device versions of MuseDiffusion/utils/decode_util.py: the batch layout and token checks and the
decode path from sampled token rows to notes, chord markers and Standard MIDI Files (split_meta_midi / restore_chord /
validation / commu's word_to_event + write_midi: csrc/decode.hip; the file itself is written by a small host writer here).
The way in - MetaToSequence, encode_notes, merge_and_mask, encode_batch (utils/encode_util.py, csrc/encode.hip) - is re-exported
here, where the reference keeps MetaToSequence and meta_to_batch; `read_midi` is `write_midi`'s counterpart.  So are the names of
utils/infill_util.py (plan_infill, splice_infill: the mask and the splice of a bar-range or per-field infill; csrc/infill.hip)."""
import os
import struct

import numpy as np
import torch

from .._lib import check, current_stream, lib, ptr, require_device
from .encode_util import (EncodedBatch, MetaToSequence, UnprocessableMidiError, chord_slots, encode_batch, encode_notes,  # noqa: F401
                          merge_and_mask)
from .infill_util import (FIELDS, INFILL_BAD_MASK, INFILL_BAD_RANGE, INFILL_NO_EOS, INFILL_OK, INFILL_OVERFLOW,  # noqa: F401
                          INFILL_STATUS_MESSAGE, InfillPlan, InfillResult, plan_infill, splice_infill)


def meta_to_batch(midi_meta_dict_or_tokens, batch_size, seq_len, device="cuda"):
    """decode_util.py:221-230: input_ids[:, :len(meta)] = meta, input_mask = 1 except [:, :len(meta) + 1] = 0 (int32).  A dict is the
    reference's argument and goes through MetaToSequence first; a sequence is the already encoded meta + chord tokens."""
    encoded_meta = midi_meta_dict_or_tokens
    if isinstance(encoded_meta, dict):
        encoded_meta = MetaToSequence().execute(encoded_meta)
    meta = torch.as_tensor(encoded_meta, dtype=torch.int32).to(device).contiguous()
    ids = torch.empty(batch_size, seq_len, device=device, dtype=torch.int32)
    mask = torch.empty_like(ids)
    check(lib().mh_meta_to_batch(ptr(meta), meta.numel(), ptr(ids), ptr(mask), batch_size, seq_len, current_stream()), "mh_meta_to_batch")
    return {"input_ids": ids, "input_mask": mask}


def validate_tokens(tokens, lengths=None):
    """[B, L] int tokens (note sequences, meta already split off) -> int32 [B, 3]: (index of the first EOS or -1 = the
    reference's "NO EOS TOKEN", validate_once passes, validate_rigidly passes; -2 where the reference's strict validator
    indexes past the end of a truncated note) - decode_util.py:73-84, :142-183, without leaving the device."""
    require_device(tokens, lengths)
    tokens = tokens.to(torch.int32).contiguous()
    B, L = tokens.shape
    lengths = None if lengths is None else lengths.to(torch.int32).contiguous()
    res = torch.empty(B, 3, device=tokens.device, dtype=torch.int32)
    check(lib().mh_validate_tokens(ptr(tokens), ptr(lengths), ptr(res), B, L, current_stream()), "mh_validate_tokens")
    return res


# ------------------------------------------------------------------------------------------------ tokens -> notes -> MIDI files
# mirror of enum mh_decode_status (include/musehip.h)
OK, NO_EOS, RESTORE_FAILED, ONCE_FAILED, STRICT_FAILED, REF_INDEXERROR, BAD_META, OVERFLOW = range(8)
STATUS_MESSAGE = {
    OK: "ok",
    NO_EOS: "NO EOS TOKEN",
    RESTORE_FAILED: "RESTORE_CHORD FROM META FAILED",
    ONCE_FAILED: "VALIDATION OF SEQUENCE FAILED",
    STRICT_FAILED: "STRICT VALIDATION OF SEQUENCE FAILED",
    REF_INDEXERROR: "the reference raises IndexError on this row (restore_chord or validate_rigidly indexes past the end)",
    BAD_META: "bpm / key / time-signature token outside its range, or a mask that sums outside [0, L]",
    OVERFLOW: "restored sequence, notes or chords exceed the capacity given (not a reference failure)",
}

TICKS_PER_BEAT = 480
TIME_SIGNATURES = ((4, 4), (3, 4), (6, 8), (12, 8))                       # tokens 627..630
_ROOTS = ("a", "a#", "b", "c", "c#", "d", "d#", "e", "f", "f#", "g", "g#")
_QUALITIES = ("", "7", "+", "dim", "m", "m7", "m7b5", "maj7", "sus4")
CHORD_NAMES = tuple(r + q for r in _ROOTS for q in _QUALITIES) + ("NN",)   # tokens 195..303
_KEY_ROOTS = ("c", "db", "d", "eb", "e", "f", "gb", "g", "ab", "a", "bb", "b")
KEY_NAMES = tuple(r + "major" for r in _KEY_ROOTS) + tuple(r + "minor" for r in _KEY_ROOTS)   # tokens 602..625
_MAJOR_SHARPS = (0, -5, 2, -3, 4, -1, -6, 1, -4, 3, -2, 5)                # sharps (+) / flats (-) of the major key on each root


def _max_row():
    return int(lib().mh_batch_max_row())


def _as_device_i32(t):
    t = torch.as_tensor(t)
    if not t.is_cuda:
        t = t.to("cuda")
    return t.to(torch.int32).contiguous()


def split_meta_midi(tokens, input_mask, ld_out=None):
    """Batch SequenceToMidi.split_meta_midi (decode_util.py:192-199) on the device: tokens / input_mask [B, L] ->
    (restored [B, ld_out] int32, zero past each row's length; lengths [B]; meta [B, 11]; status [B]).  restored / lengths / meta are
    what metric.ONNC / Controllability_* take (run/sample.py:256-262).  ld_out defaults to min(2 L, mh_batch_max_row()): n + C <= L
    tokens for a row no step of restore_chord copies twice; a longer row gets OVERFLOW."""
    require_device(tokens, input_mask)
    tokens, input_mask = tokens.to(torch.int32).contiguous(), input_mask.to(torch.int32).contiguous()
    B, L = tokens.shape
    assert input_mask.shape == tokens.shape
    ld_out = min(2 * L, _max_row()) if ld_out is None else int(ld_out)
    dev = tokens.device
    restored = torch.empty(B, ld_out, device=dev, dtype=torch.int32)
    meta = torch.empty(B, 11, device=dev, dtype=torch.int32)
    lengths, status = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().mh_restore_chord(ptr(tokens), ptr(input_mask), ptr(restored), ptr(lengths), ptr(meta), ptr(status), B, L, ld_out,
                                 current_stream()), "mh_restore_chord")
    return restored, lengths, meta, status


class DecodedRows:
    """Host side of a DecodedBatch: status [B], meta [B, 11], counts [B, 3] numpy arrays and per-row `notes[b]` [k, 4] =
    (start tick, end tick, pitch, velocity), `chords[b]` [k, 2] = (tick, chord token) - empty for rows that did not decode."""

    def __init__(self, status, meta, counts, notes, chords):
        self.status, self.meta, self.counts, self.notes, self.chords = status, meta, counts, notes, chords

    def __len__(self):
        return len(self.status)


class DecodedBatch:
    """Device tensors of one decoded batch: restored [B, ld], lengths [B], meta [B, 11], notes [B, max_notes, 4], chords
    [B, max_chords, 2], counts [B, 3] = (notes, chords, out-of-vocabulary tokens), status [B] (module constants OK ... OVERFLOW)."""

    def __init__(self, restored, lengths, packed, B, max_notes, max_chords):
        self.restored, self.lengths, self._packed = restored, lengths, packed
        self._shape = (B, max_notes, max_chords)
        o = [int(x) for x in np.cumsum([0, B, B * 3, B * 11, B * max_notes * 4, B * max_chords * 2])]
        self.status, self.counts, self.meta = packed[o[0]:o[1]], packed[o[1]:o[2]].view(B, 3), packed[o[2]:o[3]].view(B, 11)
        self.notes, self.chords = packed[o[3]:o[4]].view(B, max_notes, 4), packed[o[4]:o[5]].view(B, max_chords, 2)

    def select(self, rows):
        """rows: int64 [n] row indices on the device -> the DecodedBatch of those rows, in that order (one gather per field, no sync
        with the host)"""
        _, max_notes, max_chords = self._shape
        packed = torch.cat([t.index_select(0, rows).reshape(-1) for t in (self.status, self.counts, self.meta, self.notes, self.chords)])
        return DecodedBatch(self.restored.index_select(0, rows), self.lengths.index_select(0, rows), packed, rows.shape[0], max_notes,
                            max_chords)

    def cpu(self):
        """one device -> host copy of everything but the restored rows"""
        B, max_notes, max_chords = self._shape
        host = DecodedBatch(None, None, self._packed.cpu(), B, max_notes, max_chords)
        status, counts = host.status.numpy(), host.counts.numpy()
        ok = status == OK
        notes = [host.notes[b, :counts[b, 0]].numpy() if ok[b] else np.zeros((0, 4), np.int32) for b in range(B)]
        chords = [host.chords[b, :counts[b, 1]].numpy() if ok[b] else np.zeros((0, 2), np.int32) for b in range(B)]
        return DecodedRows(status, host.meta.numpy(), counts, notes, chords)


def decode_tokens(tokens, input_mask, strict_validation=False, ld_out=None, max_notes=None, max_chords=None):
    """SequenceToMidi.decode up to the MIDI container (decode_util.py:205-208), for a batch, on the device -> DecodedBatch.
    Validation is of the restored sequence: validate_once inside mh_decode_events, validate_rigidly (strict_validation) from
    mh_validate_tokens.  A note takes four tokens and a chord two, so the default capacities (ld // 4 and ld // 2) cannot overflow."""
    restored, lengths, meta, status = split_meta_midi(tokens, input_mask, ld_out)
    B, ld = restored.shape
    max_notes = ld // 4 + 1 if max_notes is None else int(max_notes)
    max_chords = ld // 2 + 1 if max_chords is None else int(max_chords)
    packed = torch.zeros(B * (1 + 3 + 11 + max_notes * 4 + max_chords * 2), device=restored.device, dtype=torch.int32)
    out = DecodedBatch(restored, lengths, packed, B, max_notes, max_chords)
    out.status.copy_(status)
    out.meta.copy_(meta)
    val = validate_tokens(restored, lengths) if strict_validation else None
    check(lib().mh_decode_events(ptr(restored), ptr(lengths), ptr(out.meta), ptr(val), int(bool(strict_validation)), ptr(out.notes),
                                 ptr(out.chords), ptr(out.counts), ptr(out.status), B, ld, max_notes, max_chords, current_stream()),
          "mh_decode_events")
    return out


def first_bar_shift(decoded):
    """int64 [B]: 1 where the first token of the restored row that the decoder keeps (2..559) is not BAR, else 0.  The decoder counts a
    BAR only behind the row's first kept token, so in such a row the notes in front of the first BAR fill bar 0 and the bar that BAR
    opens is bar 1, while an infill plan numbers the bars from the first BAR (bar 0) and gives the tokens before it to no bar:
    a note's start / ticks_per_bar is its infill ordinal plus this shift."""
    r = decoded.restored
    idx = torch.arange(r.shape[1], device=r.device).unsqueeze(0)
    kept = (r >= 2) & (r <= 559) & (idx < decoded.lengths.unsqueeze(1))
    first = torch.where(kept.any(1), r.gather(1, kept.int().argmax(1, keepdim=True)).squeeze(1), torch.full_like(r[:, 0], 2))
    return (first != 2).long()


def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def _track(events):
    """events: (tick, order, bytes) -> MTrk chunk with delta times and the end-of-track event"""
    body, now = b"", 0
    for tick, _, data in sorted(events, key=lambda e: (e[0], e[1])):
        body += _vlq(tick - now) + data
        now = tick
    body += b"\x00\xff\x2f\x00"
    return b"MTrk" + struct.pack(">I", len(body)) + body


def conductor_track(chords, meta):
    """track 0 of write_midi as an MTrk chunk: tempo, time signature, key signature and the chord markers (shared with
    utils.arrange_util.write_song)"""
    bpm = (int(meta[0]) - 560) * 5
    num, den = TIME_SIGNATURES[int(meta[2]) - 627]
    key = int(meta[1]) - 602
    if bpm <= 0 or not 0 <= key < 24:
        raise ValueError("write_midi: meta tokens out of range: %r" % (list(meta[:3]),))
    minor = key >= 12
    sf = _MAJOR_SHARPS[(key % 12 + 3) % 12] if minor else _MAJOR_SHARPS[key]      # a minor key shares its relative major's signature
    t0 = [(0, 0, b"\xff\x51\x03" + struct.pack(">I", int(round(60_000_000 / bpm)))[1:]),
          (0, 1, b"\xff\x58\x04" + bytes([num, den.bit_length() - 1, 24, 8])),
          (0, 2, b"\xff\x59\x02" + struct.pack(">bB", sf, int(minor)))]
    for k, (tick, tok) in enumerate(np.asarray(chords).reshape(-1, 2).tolist()):
        text = CHORD_NAMES[tok - 195].encode()
        t0.append((tick, 3 + k, b"\xff\x06" + _vlq(len(text)) + text))
    return _track(t0)


def note_events(notes, channel=0):
    """the note-on / note-off events of a note track in write_midi's order: at one tick, offs go before ons"""
    out = []
    for k, (start, end, pitch, vel) in enumerate(np.asarray(notes).reshape(-1, 4).tolist()):
        out.append((start, 2 + 2 * k + 1, bytes([0x90 | channel, pitch, vel])))
        out.append((end, 1, bytes([0x80 | channel, pitch, 0])))
    return out


def write_midi(path, notes, chords, meta):
    """Standard MIDI File, format 1, 480 ticks per beat, no third-party package.  Track 0: tempo = (bpm token - 560) * 5 BPM, time
    signature, key signature, the chord markers as text (CHORD_NAMES); track 1: program 0 on channel 0 and the notes
    (start tick, end tick, pitch, velocity).  What encoder_utils.write_midi puts into its miditoolkit container; byte equality
    with miditoolkit's dump is not claimed (the package is not a dependency) - the content is."""
    t0 = conductor_track(chords, meta)
    t1 = [(0, 0, b"\xc0\x00")] + note_events(notes)
    with open(path, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 1, 2, TICKS_PER_BEAT) + t0 + _track(t1))


def _read_vlq(data, i):
    n = 0
    while True:
        b = data[i]
        i += 1
        n = (n << 7) | (b & 0x7F)
        if not b & 0x80:
            return n, i


def read_midi(path):
    """Standard MIDI File, format 0 or 1 -> (ticks_per_beat, notes int32 [k, 4] = (start tick, end tick, pitch, velocity)) of the first
    track that holds a note, all channels together, in the order the notes START; no third-party package.  Running status is followed;
    a note-on of velocity 0 is a note-off; a note-off closes the oldest open note of its pitch and channel; a note still open at the
    end of its track is closed there.  A file that is cut short, or whose events run past their track chunk, raises ValueError.
    This is NOT miditoolkit's instrument grouping (which splits a track by channel and program and names instruments[0] the first of
    those): for the single-instrument files write_midi and ComMU produce the two agree."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"MThd" or len(data) < 14:
        raise ValueError("read_midi: %s is no Standard MIDI File" % (path,))
    hlen, fmt, ntrk, division = struct.unpack(">IHHH", data[4:14])
    if fmt > 1 or division & 0x8000:
        raise ValueError("read_midi: format %d / SMPTE time division are not supported" % fmt)
    i = 8 + hlen
    for _ in range(ntrk):
        if data[i:i + 4] != b"MTrk":
            raise ValueError("read_midi: track chunk expected at byte %d" % i)
        if i + 8 > len(data):
            raise ValueError("read_midi: %s is truncated in a track header" % (path,))
        end = i + 8 + struct.unpack(">I", data[i + 4:i + 8])[0]
        if end > len(data):
            raise ValueError("read_midi: %s is truncated: the track at byte %d says it ends at byte %d of %d" % (path, i, end, len(data)))
        try:
            notes, now = _read_track(data[i + 8:end])
        except IndexError:
            raise ValueError("read_midi: %s: an event runs past the end of the track at byte %d" % (path, i)) from None
        if notes:
            return division, np.array([[s, now if e is None else e, p, v] for s, e, p, v in notes], np.int32)
        i = end
    return division, np.zeros((0, 4), np.int32)


def _read_track(data, info=None):
    """the body of one MTrk chunk -> ([start, end or None, pitch, velocity] per note in start order, the track's last tick).  Every
    read is inside `data`: an event that runs past the chunk raises IndexError, which read_midi reports as its ValueError.
    info: a dict that takes the track's "name" (its first FF 03 event), "program" (its first program change) and "channel" (of its
    first channel message) - utils.arrange_util.read_song."""
    i, end = 0, len(data)
    now, status, running, open_notes, notes = 0, 0, 0, {}, []
    while i < end:
        delta, i = _read_vlq(data, i)
        now += delta
        if data[i] & 0x80:
            status = data[i]
            i += 1
            running = status if status < 0xF0 else 0                             # only channel messages leave a running status
        else:
            status = running
        if status == 0xFF:                                                      # meta event: type, length, data
            kind = data[i]
            n, i = _read_vlq(data, i + 1)
            if info is not None and kind == 3 and i + n <= end:
                info.setdefault("name", bytes(data[i:i + n]).decode("utf-8", "replace"))
            i += n
        elif status in (0xF0, 0xF7):                                             # system exclusive
            n, i = _read_vlq(data, i)
            i += n
        elif status >> 4 in (0xC, 0xD):
            if info is not None:
                info.setdefault("channel", status & 0xF)
                if status >> 4 == 0xC:
                    info.setdefault("program", data[i])
            i += 1
        elif status >> 4 in (0x8, 0x9):
            key, vel = (status & 0xF, data[i]), data[i + 1]
            i += 2
            if info is not None:
                info.setdefault("channel", status & 0xF)
            if status >> 4 == 0x9 and vel > 0:
                open_notes.setdefault(key, []).append(len(notes))
                notes.append([now, None, key[1], vel])
            elif open_notes.get(key):
                notes[open_notes[key].pop(0)][1] = now
        else:
            i += 2
        if i > end:                                                              # a length that points behind the chunk
            raise IndexError(i)
    return notes, now


def decode_batch(mode, sequences, input_ids_mask_ori, batch_index, previous_count, output_dir, return_indices=False,
                 strict_validation=False):
    """decode_util.py:233-384 decode_batch: the reference's signature, file names and return values; the decoding is
    decode_tokens (device or host tensors, one device -> host copy per batch).  "generation": valid rows are numbered from
    previous_count (generated_{valid_index:0>7}.midi); "modification": every valid row is named by its original index
    ({original_index:0>7}_batch{batch_index:0>5}_{index:0>4}.midi).  Returns valid_count or (valid_count, invalid indices).
    Where the reference prints each OOV token the count is printed.  A REF_INDEXERROR row raises IndexError as the reference does;
    BAD_META raises KeyError (the reference's table lookups); OVERFLOW cannot happen with the default capacities."""
    assert mode in ("generation", "modification"), "Unknown decoding mode"
    rows = decode_tokens(_as_device_i32(sequences), _as_device_i32(input_ids_mask_ori), strict_validation).cpu()
    return write_decoded_rows(mode, rows, batch_index, previous_count, output_dir, return_indices)


def write_decoded_rows(mode, rows, batch_index, previous_count, output_dir, return_indices=False):
    """The host half of decode_batch: name and write one file per valid row of a DecodedRows, report, count."""
    assert mode in ("generation", "modification"), "Unknown decoding mode"
    valid_index, invalid = previous_count, []
    for index in range(len(rows)):
        st, original_index = int(rows.status[index]), previous_count + index
        if st in (NO_EOS, RESTORE_FAILED, ONCE_FAILED, STRICT_FAILED):               # the reference's SequenceToMidiError
            if mode == "modification":
                print(f"<Warning> Batch {batch_index} Index {index} (Original: {original_index}) - Generation Failure: {STATUS_MESSAGE[st]}")
            invalid.append(index)
            continue
        if st != OK:
            where = f"Batch {batch_index} Index {index} (Original: {original_index})"
            raise {REF_INDEXERROR: IndexError, BAD_META: KeyError}.get(st, RuntimeError)(f"{STATUS_MESSAGE[st]}: {where}")
        if rows.counts[index, 2]:
            head = f"Index {valid_index}" if mode == "generation" else f"Batch {batch_index} Index {index} (Original: {original_index})"
            print(f"<Warning> {head} - OOV: {int(rows.counts[index, 2])} tokens")
        if mode == "generation":
            name = f"generated_{valid_index:0>7}.midi"
        else:
            name = f"{original_index:0>7}_batch{batch_index:0>5}_{index:0>4}.midi"
        write_midi(os.path.join(output_dir, name), rows.notes[index], rows.chords[index], rows.meta[index])
        valid_index += 1
    valid_count = len(rows) - len(invalid)
    if mode == "generation":
        print(f"\n{f' Summary of Trial {batch_index} ':=^60}\n * {valid_count} valid sequences are converted to midi into path:\n"
              f"     {os.path.abspath(output_dir)}\n * Totally {valid_index} sequences are converted.\n" + "=" * 60 + "\n")
    else:
        print(f"\n{f' Summary of Batch {batch_index} ':=^60}\n * Original index: from {previous_count} to {previous_count + len(rows)}\n"
              f" * {valid_count} valid sequences are converted to midi into path:\n     {os.path.abspath(output_dir)}\n"
              f" * {len(invalid)} sequences are invalid.\n"
              + (f" * Index (in batch {batch_index}) of invalid sequence:\n    {invalid}\n" if invalid else "") + "=" * 60 + "\n")
    return (valid_count, invalid) if return_indices else valid_count
