"""Plain-Python restatement of the interplay rule (include/musehip_arrange.h), the model csrc/arrange.hip is compared with bit for
bit.  Written from the rule's wording and NOT the way the kernel computes it: no tiles, no rewritten notes, no partial sums - a row's
counted notes are met one at a time with the counted notes of all its partners, which stand in numpy int64 columns so that a 4096-note
row stays affordable.  Everything is an integer."""
import numpy as np

OK, MASKED, BAD_COUNTS, BAD_SHIFT, MIXED = range(5)
MAX_TICK = 2 ** 29
CLAMP = 65535
TICKS_PER_BAR = {627: 1920, 628: 1440, 629: 1440, 630: 2880}
ROLE_FIRST, ROLE_LAST, DRUMS = 719, 725, 648                  # track_role tokens (meta[9]); the inst token (meta[5]) of the drum group


def counted_notes(notes, n, shift):
    """the first n notes of a list -> int64 [k, 3] = (shifted start, shifted end, pitch) of the counted ones"""
    a = np.asarray(notes, np.int64).reshape(-1, 4)[:n]
    keep = (a[:, 2] >= 0) & (a[:, 2] <= 127) & (a[:, 0] >= 0) & (a[:, 0] < a[:, 1]) & (a[:, 1] <= MAX_TICK)
    a = a[keep]
    return np.stack([a[:, 0] + shift, a[:, 1] + shift, a[:, 2]], 1)


def batch_counts(notes, counts3, meta, valid=None, song=None, shift=None):
    """[B, max_notes, 4], [B, 3], [B, 11] arrays (+ valid, song, shift [B] or None) -> dict of arrays as mha_interplay_counts fills
    them: counts int32 [B, 8], pairs int64 [B, 9], ticks int64 [B, 9], status int32 [B]"""
    B, max_notes = len(notes), np.asarray(notes).shape[1]
    n = [int(counts3[b][0]) for b in range(B)]
    s = [0 if shift is None else int(shift[b]) for b in range(B)]
    g = [0 if song is None else int(song[b]) for b in range(B)]
    on = [True if valid is None else int(valid[b]) != 0 for b in range(B)]
    in_range = [on[b] and 0 <= n[b] <= max_notes and 0 <= s[b] <= MAX_TICK for b in range(B)]
    counts, pairs, ticks = np.zeros((B, 8), np.int32), np.zeros((B, 9), np.int64), np.zeros((B, 9), np.int64)
    status = np.zeros(B, np.int32)
    lists = {}

    def counted(c):
        if c not in lists:
            lists[c] = counted_notes(notes[c], n[c], s[c])
        return lists[c]

    for b in range(B):
        if not on[b]:
            status[b] = MASKED
        elif not 0 <= n[b] <= max_notes:
            status[b] = BAD_COUNTS
        elif not 0 <= s[b] <= MAX_TICK:
            status[b] = BAD_SHIFT
        if status[b]:
            continue
        partners = [c for c in range(B) if c != b and g[c] == g[b] and in_range[c]]
        if any(int(meta[c][i]) != int(meta[b][i]) for c in partners for i in range(3)):
            status[b] = MIXED
            continue
        mine = counted(b)
        theirs = np.concatenate([counted(c) for c in partners]) if partners else np.zeros((0, 3), np.int64)
        accompanied = 0
        for start, end, pitch in mine.tolist():
            o = np.minimum(end, theirs[:, 1]) - np.maximum(start, theirs[:, 0])
            together = o > 0
            if not together.any():
                continue
            accompanied += 1
            common = np.minimum(o[together], CLAMP)
            other = theirs[together, 2]
            d = np.abs(pitch - other) % 12
            ic = np.minimum(d, 12 - d)
            for col in range(7):
                pairs[b, col] += int((ic == col).sum())
                ticks[b, col] += int(common[ic == col].sum())
            for col, rel in ((7, pitch < other), (8, pitch > other)):
                pairs[b, col] += int(rel.sum())
                ticks[b, col] += int(common[rel].sum())
        counts[b, :4] = [len(mine), n[b] - len(mine), len(partners), accompanied]
    return dict(counts=counts, pairs=pairs, ticks=ticks, status=status)


def first_bar_shift(restored, length):
    """1 where the first token of the row that the decoder keeps (2..559) is not BAR (2), else 0"""
    for tok in list(restored)[:int(length)]:
        if 2 <= int(tok) <= 559:
            return int(int(tok) != 2)
    return 0


def align_shift(first, ok, song, meta):
    """lists per row: first = first_bar_shift, ok = the row decoded -> ticks per row: one bar for a row whose first BAR opens bar 0
    when a decoded row of its song has notes in front of its first BAR"""
    out = []
    for b in range(len(first)):
        late = any(ok[c] and first[c] == 1 and song[c] == song[b] for c in range(len(first)))
        out.append(TICKS_PER_BAR.get(int(meta[b][2]), 0) if late and first[b] == 0 else 0)
    return out


class Totals:
    """evaluation.InterplayTotals without a device: Python ints"""

    def __init__(self):
        self.ticks, self.pairs = [0] * 9, [0] * 9
        self.role_ticks, self.role_pairs = [[0] * 9 for _ in range(8)], [[0] * 9 for _ in range(8)]
        self.rows = self.notes = self.accompanied = self.songs = 0

    def update(self, out, meta, songs):
        for b in range(len(out["status"])):
            if out["status"][b] != OK:
                continue
            role = int(meta[b][9])
            r = role - ROLE_FIRST if ROLE_FIRST <= role <= ROLE_LAST else 7
            for c in range(9):
                self.ticks[c] += int(out["ticks"][b, c])
                self.pairs[c] += int(out["pairs"][b, c])
                self.role_ticks[r][c] += int(out["ticks"][b, c])
                self.role_pairs[r][c] += int(out["pairs"][b, c])
            self.rows += 1
            self.notes += int(out["counts"][b, 0])
            self.accompanied += int(out["counts"][b, 3])
        self.songs += songs

    def vector(self):
        flat = lambda m: [x for row in m for x in row]  # noqa: E731
        return self.ticks + self.pairs + flat(self.role_ticks) + flat(self.role_pairs) + [self.rows, self.notes, self.accompanied, self.songs]
