"""The way INTO the model: a meta dict, a chord progression and a note list (or a MIDI file) -> the token rows sampling and
training take.  The inverse of utils/decode_util.py's decode path:

    MetaToSequence     meta dict -> 11 meta tokens + the chord part (MuseDiffusion/utils/decode_util.py:16-50 over commu's MetaEncoder,
                       commu/preprocessor/encoder/meta.py) - host only, no third-party package
    encode_notes       notes + time base + chord progression -> event words (commu's EventSequenceEncoder.encode, encoder.py:21-69
                       and encoder_utils.py:184-368, from the note list onward) - csrc/encode.hip, one block per row
    merge_and_mask     meta tokens + words -> input_ids / input_mask / length (MuseDiffusion/data/preprocess.py:30-61) - csrc/encode.hip
    encode_batch       (notes or MIDI path, meta dict) pairs -> the `cond` dict of collate_batches

The string work (chord names -> ids and tokens) is the host's; all arithmetic, sorting and compaction is the kernels'."""
import math

import numpy as np
import torch

from .._lib import check, current_stream, lib, ptr, require_device

# mirror of enum mh_encode_status (include/musehip.h)
OK, EMPTY, NO_CHORDS, BAD_TIMEBASE, BAD_CHORDS, OVERFLOW = range(6)
STATUS_MESSAGE = {
    OK: "ok",
    EMPTY: "no notes (the reference raises IndexError)",
    NO_CHORDS: "empty chord progression (the reference's extract_events returns None and encode fails)",
    BAD_TIMEBASE: "fewer than 128 ticks per bar, or a time base that is no positive number (the reference divides by zero)",
    BAD_CHORDS: "the number of chord slots is no multiple of the chords per bar (not a reference failure: np.array_split would split unevenly)",
    OVERFLOW: "more notes, chord slots, events or words than the capacity given (not a reference failure)",
}

# ------------------------------------------------------------------------------------------------------------ meta -> tokens
UNKNOWN = "unknown"
META_FIELDS = ("bpm", "audio_key", "time_signature", "pitch_range", "num_measures", "inst", "genre", "min_velocity", "max_velocity",
               "track_role", "rhythm")                                    # MidiMeta's field order = the order of the eleven tokens
# commu/preprocessor/encoder/event_tokens.py:308-329: the "unknown" token of each field; a known value is offset + 1 + its index
_OFFSET = dict(bpm=560, audio_key=601, time_signature=626, pitch_range=630, num_measures=638, inst=641, genre=650, velocity=653,
               track_role=719, rhythm=726)
_KEY_ROOTS = ("c", "c#", "d", "d#", "e", "f", "f#", "g", "g#", "a", "a#", "b")
_FLAT_OF = {"c#": "db", "d#": "eb", "f#": "gb", "g#": "ab", "a#": "bb"}
KEY_MAP = {}
for _m, _mode in enumerate(("major", "minor")):
    for _i, _r in enumerate(_KEY_ROOTS):
        KEY_MAP[_r + _mode] = 12 * _m + _i
        if _r in _FLAT_OF:
            KEY_MAP[_FLAT_OF[_r] + _mode] = 12 * _m + _i
TIME_SIG_MAP = {"4/4": 0, "3/4": 1, "6/8": 2, "12/8": 3}
PITCH_RANGE_MAP = {n: i for i, n in enumerate(("very_low", "low", "mid_low", "mid", "mid_high", "high", "very_high"))}
_INST_GROUPS = (
    "acoustic_piano electric_piano harpsichord keyboard organ",
    "accordion synth_lead",
    "bell celesta glockenspiel marimba synth_bell vibraphone xylophone orgel",
    "acoustic_bass acoustic_guitar banjo electric_bass electric_guitar_clean electric_guitar_distortion harp mandolin nylon_guitar oud "
    "sitar synth_bass synth_bass_808 synth_bass_wobble ukulele zither yanggeum",
    "fiddle pad_synth string_cello string_double_bass string_ensemble string_viola string_violin synth_pad",
    "bassoon brass_ensemble clarinet flute horn oboe recorder trombone trumpet tuba synth_brass sax bamboo_flute",
    "drums_full drums_tops percussion timpani",
    "choir synth_pluck synth_voice whistle",
    "vocal",
)
INST_MAP = {n: i for i, g in enumerate(_INST_GROUPS) for n in g.split()}
GENRE_MAP = {"newage": 0, "cinematic": 1}
TRACK_ROLE_MAP = {n: i for i, n in enumerate(("main_melody", "sub_melody", "accompaniment", "bass", "pad", "riff"))}
RHYTHM_MAP = {"standard": 0, "triplet": 1}
_MAPPED = dict(audio_key=(KEY_MAP, "audio key"), time_signature=(TIME_SIG_MAP, "ts"), pitch_range=(PITCH_RANGE_MAP, "pitch range"),
               inst=(INST_MAP, "inst"), genre=(GENRE_MAP, "genre"), track_role=(TRACK_ROLE_MAP, "track role"), rhythm=(RHYTHM_MAP, "rhythm"))

_ROOTS = ("a", "a#", "b", "c", "c#", "d", "d#", "e", "f", "f#", "g", "g#")
_QUALITIES = ("", "7", "+", "dim", "m", "m7", "m7b5", "maj7", "sus4")
CHORD_NAMES = tuple(r + q for r in _ROOTS for q in _QUALITIES) + ("NN",)   # tokens 195..303 (== decode_util.CHORD_NAMES)


class UnprocessableMidiError(ValueError):
    """commu.preprocessor.utils.exceptions.UnprocessableMidiError: a meta value no token stands for"""


def _encode_field(name, value):
    if name == "num_measures":                                           # meta.py:156-173: "unknown" is an error here
        if value == UNKNOWN:
            raise UnprocessableMidiError("Unprocessable midi")
        n = math.floor(float(value))
        if n in (4, 5, 8, 9, 16, 17):
            return _OFFSET[name] + (0 if n < 8 else 1 if n < 16 else 2)
        raise UnprocessableMidiError("num measures ValueError: %d" % n)
    group = "velocity" if name.endswith("velocity") else name
    if value == UNKNOWN:
        return _OFFSET[group]
    if name == "bpm":                                                    # min(bpm, 200) // 5, at least 1; no + 1: bpm 0 is not a value
        return _OFFSET[name] + (min(int(value), 200) // 5 or 1)
    if name == "min_velocity":
        return _OFFSET[group] + 1 + math.floor(int(value) / 2)
    if name == "max_velocity":
        return _OFFSET[group] + 1 + math.ceil(int(value) / 2)
    table, label = _MAPPED[name]
    if value not in table:
        raise UnprocessableMidiError("%s KeyError: %s" % (label, value))
    return _OFFSET[name] + 1 + table[value]


class MetaToSequence:
    """MuseDiffusion/utils/decode_util.py:16-50 without `commu` and `pydantic`: the eleven meta fields in MidiMeta's order with the
    maps of commu's constants.py, then the chord part.  "unknown" gives the field's own unknown token, except for num_measures, where
    it is an error as in the reference; num_measures accepts 4 / 5, 8 / 9 and 16 / 17 (after floor) only."""

    def __init__(self):
        self.chord_map = {n[0].upper() + n[1:]: CHORD_NAMES.index(n) + 195 for n in CHORD_NAMES}

    def encode_chord(self, chord_progression):
        """:25-39, quirks kept: eight slots per bar whatever the time signature; a bar is 432 + its first chord's token, and a change
        inside the bar appends its position 432 + 16 i ONLY (the changed chord's own token is not written)"""
        assert len(chord_progression) % 8 == 0
        out = []
        for idx in range(0, len(chord_progression), 8):
            out += [432, self.chord_map[chord_progression[idx]]]
            recent = chord_progression[idx]
            for i in range(1, 8):
                if recent != chord_progression[idx + i]:
                    out.append(432 + i * 16)
                    recent = chord_progression[idx + i]
        return out

    def encode_meta(self, midi_meta):
        """a mapping (or an object with the eleven attributes) -> eleven tokens"""
        get = midi_meta.__getitem__ if hasattr(midi_meta, "__getitem__") else (lambda k: getattr(midi_meta, k))
        return [_encode_field(name, get(name)) for name in META_FIELDS]

    def execute(self, input_data):
        return self.encode_meta(input_data) + self.encode_chord(input_data["chord_progression"].split("-"))

    def __call__(self, *args, **kwargs):
        return self.execute(*args, **kwargs)


# ------------------------------------------------------------------------------------------------- chord names -> kernel input
def _chord_vocabulary():
    """event2word's chord entries: the 109 base chords, add_flat_chord2map's flat roots, abstract_chord_types' aliases on natural roots
    (encoder_utils.py:59-182).  Keys keep the reference's spelling: 'mM7' has a capital M, so no lowercased name ever finds it."""
    v = {n: 195 + i for i, n in enumerate(CHORD_NAMES)}
    base_of = {"": "", "maj": "", "6": "", "maj7": "maj7", "add2": "maj7", "sus2": "maj7", "7": "7", "dim": "dim", "dim7": "dim", "+": "+",
               "m": "m", "m6": "m", "mM7": "m", "m7": "m7", "madd2": "m7", "sus4": "sus4", "7sus4": "sus4", "m7b5": "m7b5"}
    for flat, sharp in (("ab", "g#"), ("bb", "a#"), ("db", "c#"), ("eb", "d#"), ("gb", "f#")):
        for scale, base in base_of.items():
            v[flat + scale] = v[sharp + base]
    for root in "abcdefg":
        for scale in ("7sus4", "m6", "sus2", "add2", "dim7", "6", "madd2", "mM7"):
            v[root + scale] = v[root + {"mM7": "m7", "madd2": "m7", "m6": "m"}.get(scale, base_of[scale])]
    return v


CHORD_VOCABULARY = _chord_vocabulary()


def chord_slots(names):
    """chord names, one per slot (eighth note) -> int32 [n, 2] = (name id, token) for mh_encode_events.  Ids are equal where the
    lowercased full names are (detect_chord compares the whole string, slash bass included); the token is event2word of the
    lowercased name cut at '/' and '(', or -1 where the reference prints "OOV"."""
    ids, out = {}, np.zeros((len(names), 2), np.int32)
    for k, name in enumerate(names):
        low = str(name).lower()
        out[k] = ids.setdefault(low, len(ids)), CHORD_VOCABULARY.get(low.split("/")[0].split("(")[0], -1)
    return out


# --------------------------------------------------------------------------------------------------------- the device kernels
def _i32(t, device):
    return torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()


class EncodedRows:
    """Host side of an EncodedBatch: status [B], counts [B, 2], lengths [B] numpy arrays and `words[b]`, empty unless status[b] is OK"""

    def __init__(self, status, counts, lengths, words):
        self.status, self.counts, self.lengths, self.words = status, counts, lengths, words

    def __len__(self):
        return len(self.status)


class EncodedBatch:
    """Device tensors of one encoded batch: words [B, ld] (ending in EOS, zero past lengths[b]), lengths [B], counts [B, 2] =
    (events, "OOV" lines the reference would print), status [B] (module constants OK ... OVERFLOW)."""

    def __init__(self, words, lengths, counts, status):
        self.words, self.lengths, self.counts, self.status = words, lengths, counts, status

    def cpu(self):
        words, lengths = self.words.cpu().numpy(), self.lengths.cpu().numpy()
        return EncodedRows(self.status.cpu().numpy(), self.counts.cpu().numpy(), lengths, [words[b, :lengths[b]] for b in range(len(lengths))])


def encode_notes(notes, n_notes, params, slots, n_slots, ld=None, device="cuda"):
    """EventSequenceEncoder.encode from the note list onward, for a batch, on the device -> EncodedBatch.
    notes [B, max_notes, 4] = (start tick, end tick, pitch, velocity), the layout decode_tokens writes; n_notes [B];
    params [B, 5] = (ticks_per_beat, numerator, denominator, ceil(num_measures), is_incomplete_measure as 0 / 1);
    slots [B, max_slots, 2] = chord_slots() per row, zero padded; n_slots [B].  ld: the width of `words` (default and at most
    mh_batch_max_row()); a row that needs more gets OVERFLOW."""
    notes, n_notes, params = _i32(notes, device), _i32(n_notes, device), _i32(params, device)
    slots, n_slots = _i32(slots, device), _i32(n_slots, device)
    require_device(notes)
    B, max_notes = notes.shape[0], notes.shape[1]
    assert notes.shape == (B, max_notes, 4) and params.shape == (B, 5) and slots.shape[0] == B and slots.shape[2] == 2
    assert n_notes.shape == (B,) and n_slots.shape == (B,)
    ld = int(lib().mh_batch_max_row()) if ld is None else int(ld)
    words = torch.empty(B, ld, device=notes.device, dtype=torch.int32)
    lengths, status = torch.empty(B, device=notes.device, dtype=torch.int32), torch.empty(B, device=notes.device, dtype=torch.int32)
    counts = torch.empty(B, 2, device=notes.device, dtype=torch.int32)
    check(lib().mh_encode_events(ptr(notes), ptr(n_notes), ptr(params), ptr(slots), ptr(n_slots), ptr(words), ptr(lengths), ptr(counts),
                                 ptr(status), B, max_notes, slots.shape[1], ld, current_stream()), "mh_encode_events")
    return EncodedBatch(words, lengths, counts, status)


def merge_and_mask(src, words, lengths, status=None, src_len=None):
    """helper_tokenize's merge_and_mask (data/preprocess.py:36-56) per row, on the device: src [B, S] meta tokens (src_len [B] of them,
    default S), words [B, ld] / lengths [B] as encode_notes returns them -> ({'input_ids', 'input_mask'} ragged int32 values,
    offsets int64 [B + 1], length [B], status [B]): what collate_batches and Corruptions take.  The chord tokens (195..303) and the
    token before each move from the words into the prefix; a row whose `status` is not OK gets length 0 and keeps its status."""
    require_device(words)
    dev = words.device
    words, lengths, src = words.to(torch.int32).contiguous(), _i32(lengths, dev), _i32(src, dev)
    B, ld = words.shape
    S = src.shape[1]
    assert src.shape == (B, S) and lengths.shape == (B,)
    status_in = None if status is None else _i32(status, dev)
    src_len = None if src_len is None else _i32(src_len, dev)
    cap = B * (S + 1 + 2 * ld)                                           # no row can be longer: each token is gathered at most twice
    ids, mask = torch.empty(cap, device=dev, dtype=torch.int32), torch.empty(cap, device=dev, dtype=torch.int32)
    offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    length, status_out = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().mh_merge_and_mask(ptr(src), ptr(src_len), ptr(words), ptr(lengths), ptr(status_in), ptr(ids), ptr(mask), ptr(offsets),
                                  ptr(length), ptr(status_out), B, S, ld, cap, current_stream()), "mh_merge_and_mask")
    return {"input_ids": ids, "input_mask": mask}, offsets, length, status_out


def pack_items(notes_list, params_list, names_list):
    """per-row host data -> the padded arrays encode_notes takes (numpy): notes, n_notes, params, slots, n_slots"""
    B = len(notes_list)
    notes_list = [np.asarray(n, np.int32).reshape(-1, 4) for n in notes_list]
    slot_list = [chord_slots(n) for n in names_list]
    notes = np.zeros((B, max(1, max(len(n) for n in notes_list)), 4), np.int32)
    slots = np.zeros((B, max(1, max(len(s) for s in slot_list)), 2), np.int32)
    for b in range(B):
        notes[b, :len(notes_list[b])] = notes_list[b]
        slots[b, :len(slot_list[b])] = slot_list[b]
    return (notes, np.array([len(n) for n in notes_list], np.int32), np.asarray(params_list, np.int32).reshape(B, 5), slots,
            np.array([len(s) for s in slot_list], np.int32))


def encode_batch(items, seq_len, device="cuda"):
    """items: (notes [k, 4] or the path of a MIDI file, meta dict) pairs -> (cond, report).  The meta dict holds MetaToSequence's
    fields and 'chord_progression' ("C-C-Am-..." one name per eighth note), and optionally 'is_incomplete_measure' (default False) and,
    for note arrays, 'ticks_per_beat' (default 480; a file brings its own).  cond = collate_batches' dict ('input_ids', 'input_mask',
    'length', [kept rows, seq_len]) of the rows that encoded and are at most seq_len long (helper_filter, preprocess.py:73-81);
    sampling.modify or a training step takes it unchanged.  report: 'kept' (indices into items), 'status' and 'length' of every item,
    'oov' ("OOV" lines per item)."""
    from ..data.wrapper import collate_batches
    from .decode_util import read_midi
    m2s = MetaToSequence()
    notes_list, params_list, names_list, src = [], [], [], []
    for music, meta in items:
        tpb = int(meta.get("ticks_per_beat", 480))
        if isinstance(music, (str, bytes)) or hasattr(music, "__fspath__"):
            tpb, music = read_midi(music)
        src.append(m2s.encode_meta(meta))
        num, den = (int(x) for x in str(meta["time_signature"]).split("/"))
        params_list.append((tpb, num, den, math.ceil(float(meta["num_measures"])), int(bool(meta.get("is_incomplete_measure", False)))))
        notes_list.append(music)
        names_list.append([n for n in str(meta["chord_progression"]).split("-") if n] if meta.get("chord_progression") else [])
    enc = encode_notes(*pack_items(notes_list, params_list, names_list), device=device)
    fields, offsets, length, status = merge_and_mask(torch.tensor(src, dtype=torch.int32), enc.words, enc.lengths, enc.status)
    cond = collate_batches(fields, offsets, seq_len)
    length_h, status_h = length.cpu().numpy(), status.cpu().numpy()
    kept = np.nonzero((status_h == OK) & (length_h <= seq_len))[0]
    sel = torch.from_numpy(kept).to(length.device)
    cond = {k: v.index_select(0, sel) for k, v in cond.items()}
    return cond, dict(kept=kept, status=status_h, length=length_h, oov=enc.counts[:, 1].cpu().numpy())
