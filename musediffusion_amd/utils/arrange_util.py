"""From single tracks to songs.  A ComMU piece is a stack of tracks that share one chord progression, tempo, key and time signature and
differ in role and instrument; the reference generates, decodes and writes one track at a time.  Not in the reference:
`arrangement_batch` builds the batch of the tracks of several songs (one meta_to_batch per track, rows gathered song-major),
`align_shift` puts the first BAR of every decoded track of a song on one tick, `write_song` writes the tracks of a song into ONE
Standard MIDI File (format 1: write_midi's conductor track, then a named track per row with its program and channel) and `read_song`
reads such a file back.  How the tracks of a song fit each other is metric.interplay_counts (csrc/arrange.hip)."""
import struct

import numpy as np
import torch

from . import decode_util as du
from .encode_util import META_FIELDS, TRACK_ROLE_MAP

TRACK_OVERRIDES = ("inst", "track_role", "pitch_range", "min_velocity", "max_velocity")
# General MIDI programs of the inst tokens 641 (unknown), 642..650 (encode_util._INST_GROUPS: keys, leads, mallets, plucked strings,
# bowed strings and pads, winds, drums, voices, vocal): piano, piano, accordion, vibraphone, nylon guitar, string ensemble, brass
# section, (drums: no program, channel 9), choir aahs, synth voice
INST_PROGRAMS = {641: 0, 642: 0, 643: 21, 644: 11, 645: 24, 646: 48, 647: 61, 648: 0, 649: 52, 650: 54}
DRUMS_INST, DRUM_CHANNEL = 648, 9
PLUCKED_INST, BASS_ROLE, BASS_PROGRAM = 645, 723, 32                      # a bass role on the group that holds the basses: acoustic bass
PITCHED_CHANNELS = tuple(c for c in range(16) if c != DRUM_CHANNEL)
ROLE_NAMES = ("unknown",) + tuple(sorted(TRACK_ROLE_MAP, key=TRACK_ROLE_MAP.get))   # tokens 719..725
_INST_FIELD, _ROLE_FIELD = META_FIELDS.index("inst"), META_FIELDS.index("track_role")


def arrangement_batch(base_meta, tracks, n_songs, seq_len, device="cuda"):
    """base_meta: a meta dict with a chord progression (meta_to_batch's); tracks: a list of dicts, each overriding `inst`,
    `track_role`, `pitch_range`, `min_velocity` or `max_velocity` -> (cond, song, track): cond = {'input_ids', 'input_mask'}
    [n_songs * len(tracks), seq_len] with the rows song-major (song 0's tracks, song 1's tracks, ...), song and track int32 [B]: the
    song and the index into `tracks` of every row.  One meta_to_batch per track and a row gather."""
    if not tracks or n_songs < 1:
        raise ValueError("arrangement_batch: at least one track and one song")
    for t in tracks:
        unknown = sorted(set(t) - set(TRACK_OVERRIDES))
        if unknown:
            raise ValueError("arrangement_batch: a track overrides %s, not %s" % (", ".join(TRACK_OVERRIDES), ", ".join(unknown)))
    T = len(tracks)
    per_track = [du.meta_to_batch({**base_meta, **t}, n_songs, seq_len, device) for t in tracks]
    song = torch.arange(n_songs, device=device, dtype=torch.int32).repeat_interleave(T)
    track = torch.arange(T, device=device, dtype=torch.int32).repeat(n_songs)
    rows = (track.long() * n_songs + song.long())                         # row (song s, track t) of the tracks' batches laid end to end
    cond = {k: torch.cat([c[k] for c in per_track]).index_select(0, rows) for k in ("input_ids", "input_mask")}
    return cond, song, track


def candidate_batch(base_meta, tracks, n_songs, seq_len, candidates, device="cuda"):
    """arrangement_batch with every track of every song `candidates` times: (cond, song, track, cand) with the rows in the candidate
    layout of include/musehip_choose.h - row (s * T + t) * K + k is candidate k of track t of song s, T = len(tracks), K =
    candidates; song, track and cand int32 [n_songs * T * K].  The K candidates of a track start from the same row and differ in
    what the sampler draws.  One meta_to_batch per track and a row gather."""
    K = int(candidates)
    if not tracks or n_songs < 1 or K < 1:
        raise ValueError("candidate_batch: at least one track, one song and one candidate")
    for t in tracks:
        unknown = sorted(set(t) - set(TRACK_OVERRIDES))
        if unknown:
            raise ValueError("candidate_batch: a track overrides %s, not %s" % (", ".join(TRACK_OVERRIDES), ", ".join(unknown)))
    T = len(tracks)
    per_track = [du.meta_to_batch({**base_meta, **t}, n_songs * K, seq_len, device) for t in tracks]
    row = torch.arange(n_songs * T * K, device=device, dtype=torch.int64)
    song, track, cand = row // (T * K), row // K % T, row % K
    rows = track * (n_songs * K) + song * K + cand                       # of the tracks' batches laid end to end
    cond = {k: torch.cat([c[k] for c in per_track]).index_select(0, rows) for k in ("input_ids", "input_mask")}
    return cond, song.to(torch.int32), track.to(torch.int32), cand.to(torch.int32)


def _bar_ticks(meta):
    """the ticks of one bar per row by its time-signature token meta[2]: 1920, 1440, 1440 or 2880; 0 for any other token"""
    ts = meta[:, 2]
    beats = torch.where(ts == 627, 4, torch.where(ts == 630, 6, torch.where((ts == 628) | (ts == 629), 3, 0)))
    return beats * du.TICKS_PER_BEAT


def anchor_shift(decoded):
    """decoded: a DecodedBatch -> int32 [B] ticks: one bar for a row that decoded OK and whose first kept token is its first BAR
    (du.first_bar_shift == 0), else 0.  align_shift moves such a row only when a row of its song has notes in front of its first
    BAR, so a row's shift depends on the other rows; this one is absolute - every first BAR lands on the tick of bar 1 - so the
    overlap of two candidate rows does not depend on which other candidates are chosen.  On the rows of a song that decoded it
    differs from align_shift by one constant (0 or one bar).  Torch operations only, no sync with the host."""
    f = du.first_bar_shift(decoded)
    bar = _bar_ticks(decoded.meta)
    return torch.where((f == 0) & (decoded.status == du.OK), bar, torch.zeros_like(bar)).to(torch.int32)


def align_shift(decoded, song):
    """decoded: a DecodedBatch; song [B]: the song of every row -> int32 [B] ticks to add to a row's notes so that the first BAR of
    every track of a song lands on one tick.  f = du.first_bar_shift: a row with f == 1 has notes in front of its first BAR, which
    fill bar 0, and its first BAR opens bar 1.  A row with f == 0 gets one bar (1920, 1440, 1440 or 2880 ticks by meta[2]) if any
    decoded row of its song has f == 1; every other row gets 0.  Torch operations only, no sync with the host."""
    f = du.first_bar_shift(decoded)
    song = torch.as_tensor(song).to(f.device)
    late = (f == 1) & (decoded.status == du.OK)
    waits = ((song.unsqueeze(1) == song.unsqueeze(0)) & late.unsqueeze(0)).any(1) & (f == 0)
    ts = decoded.meta[:, 2]
    beats = torch.where(ts == 627, 4, torch.where(ts == 630, 6, torch.where((ts == 628) | (ts == 629), 3, 0)))
    return torch.where(waits, beats * du.TICKS_PER_BEAT, torch.zeros_like(beats)).to(torch.int32)


def track_program(meta):
    """a row's eleven meta tokens -> (General MIDI program, is a drum row)"""
    inst, role = int(meta[_INST_FIELD]), int(meta[_ROLE_FIELD])
    if inst == PLUCKED_INST and role == BASS_ROLE:
        return BASS_PROGRAM, False
    return INST_PROGRAMS.get(inst, 0), inst == DRUMS_INST


def track_name(meta, index):
    """the default name of a track: its role and its index in the song"""
    role = int(meta[_ROLE_FIELD]) - 719
    return "%s_%d" % (ROLE_NAMES[role] if 0 <= role < len(ROLE_NAMES) else "unknown", index)


def write_song(path, tracks, chords, meta, shifts, names=None):
    """tracks: per track its notes [k, 4] = (start tick, end tick, pitch, velocity); chords [k, 2] = (tick, chord token): the song's
    markers; meta [T, 11]: the tracks' meta tokens (the first row's bpm, key and time signature are the song's); shifts: ticks added
    to each track's notes (align_shift); names: per track, default track_name.  Standard MIDI File, format 1: track 0 is exactly
    write_midi's conductor track; then one MTrk per track - its name (FF 03), a program change (track_program) and the shifted notes
    in write_midi's event order.  Drum rows go on channel 9, pitched rows take channels 0..8 and 10..15 in order; more than 15
    pitched rows raise ValueError."""
    meta = np.asarray(meta).reshape(-1, 11)
    if not (len(tracks) == len(meta) == len(shifts)) or (names is not None and len(names) != len(tracks)) or not len(tracks):
        raise ValueError("write_song: one meta row, one shift and one name per track, at least one track")
    programs = [track_program(m) for m in meta]
    if sum(1 for _, drums in programs if not drums) > len(PITCHED_CHANNELS):
        raise ValueError("write_song: %d pitched tracks, a file has %d channels for them" % (
            sum(1 for _, drums in programs if not drums), len(PITCHED_CHANNELS)))
    chunks, free = [du.conductor_track(chords, meta[0])], iter(PITCHED_CHANNELS)
    for k, (notes, (program, drums)) in enumerate(zip(tracks, programs)):
        channel = DRUM_CHANNEL if drums else next(free)
        name = (track_name(meta[k], k) if names is None else str(names[k])).encode()
        shifted = np.asarray(notes, np.int64).reshape(-1, 4).copy()
        shifted[:, :2] += int(shifts[k])
        events = [(0, -1, b"\xff\x03" + du._vlq(len(name)) + name), (0, 0, bytes([0xC0 | channel, program]))]
        chunks.append(du._track(events + du.note_events(shifted, channel)))
    with open(path, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 1, len(chunks), du.TICKS_PER_BEAT) + b"".join(chunks))


def read_song(path):
    """Standard MIDI File, format 1 -> (ticks_per_beat, [(name, channel, program, notes int32 [k, 4]) per track that holds a channel
    message, in file order]): write_song's counterpart, a sibling of read_midi with its rules for notes (running status, note-on of
    velocity 0, the oldest open note closes first, a note open at the end of its track closes there) and its ValueErrors.  name is
    None for a track without a name event, program None for one without a program change."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"MThd" or len(data) < 14:
        raise ValueError("read_song: %s is no Standard MIDI File" % (path,))
    hlen, fmt, ntrk, division = struct.unpack(">IHHH", data[4:14])
    if fmt > 1 or division & 0x8000:
        raise ValueError("read_song: format %d / SMPTE time division are not supported" % fmt)
    i, out = 8 + hlen, []
    for _ in range(ntrk):
        if data[i:i + 4] != b"MTrk" or i + 8 > len(data):
            raise ValueError("read_song: track chunk expected at byte %d" % i)
        end = i + 8 + struct.unpack(">I", data[i + 4:i + 8])[0]
        if end > len(data):
            raise ValueError("read_song: %s is truncated: the track at byte %d says it ends at byte %d of %d" % (path, i, end, len(data)))
        info = {}
        try:
            notes, now = du._read_track(data[i + 8:end], info)
        except IndexError:
            raise ValueError("read_song: %s: an event runs past the end of the track at byte %d" % (path, i)) from None
        if "channel" in info:
            arr = np.array([[s, now if e is None else e, p, v] for s, e, p, v in notes], np.int32).reshape(-1, 4)
            out.append((info.get("name"), info["channel"], info.get("program"), arr))
        i = end
    return division, out
