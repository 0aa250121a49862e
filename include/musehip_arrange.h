/* musehip_arrange.h - the interplay counts of libmusehip.so / libmusehip_dbg.so (csrc/arrange.hip).
 *
 * An eleventh header beside musehip.h, musehip_data.h, musehip_eval.h, musehip_stats.h, musehip_infill.h, musehip_harmony.h,
 * musehip_grammar.h, musehip_region.h, musehip_solver.h and musehip_structure.h: do the tracks of one song fit each other?  A ComMU
 * piece is a stack of tracks (main melody, sub melody, accompaniment, bass, pad, riff) over one chord progression; every other
 * statistic of this library looks at one row.  Here the rows of a batch are grouped into songs and every note of a row is met with
 * every note of the row's partners in time: which intervals sound together and for how long, which row lies below.  The input is
 * what mh_decode_events leaves on the device, the work is an all-pairs join of note lists and lives here under the prefix mha_.
 * Everything else is shared: mh_stream_t, the mh_status return codes, and the error text, which is read through mh_last_error().
 *
 * The rule, per row b with n = counts3[b, 0] notes (start tick, end tick, pitch, velocity), s_b = shift[b] (0 when shift is NULL)
 * and g_b = song[b] (one song when song is NULL; any int32 is an ordinary id):
 *   1 in range       row c is IN RANGE iff valid[c] != 0 (every row when valid is NULL), 0 <= n_c <= max_notes and
 *                    0 <= s_c <= 2^29.
 *   2 partners       the partners of b are the rows c != b with g_c == g_b that are in range.  Whether c is itself MIXED (step 3)
 *                    plays no part.
 *   3 status         tried in this order: MHA_MASKED (valid[b] == 0), MHA_BAD_COUNTS (n outside [0, max_notes]), MHA_BAD_SHIFT
 *                    (s_b outside [0, 2^29]), MHA_MIXED (some partner differs from b in meta[., 0], meta[., 1] or meta[., 2]: bpm,
 *                    key or time signature - the rows are not one song), MHA_OK.  A song with one odd row is MIXED in every row.
 *                    A row that is not MHA_OK gets zeros in every output and its list is not read.
 *   4 counted notes  a note is COUNTED iff 0 <= pitch <= 127 and 0 <= start < end <= 2^29; every other note among a row's n is
 *                    SKIPPED: counted as such and otherwise ignored, in b and in its partners alike.  The time of a counted note
 *                    is [start + s, end + s) with its row's s; velocity is not read.
 *   5 together       counted note x of b and counted note y of a partner SOUND TOGETHER iff
 *                    o = min(end_x, end_y) - max(start_x, start_y) > 0 in shifted times; notes that only touch do not.
 *   6 columns        a pair that sounds together adds 1 to out_pairs[b, col] and min(o, 65535) to out_ticks[b, col] for each
 *                    column that applies: col = min(d, 12 - d) with d = |p_x - p_y| mod 12, the interval class 0..6; col 7 when
 *                    p_x < p_y (this row is below); col 8 when p_x > p_y (this row is above).
 *   7 counts         out_counts[b] = (counted, skipped, partners, accompanied, 0, 0, 0, 0); accompanied = the counted notes of b
 *                    that sound together with at least one partner note.
 * Every output is an integer: the order of a row's notes, the order of the rows and the launch geometry change no output bit. */
#ifndef MUSEHIP_ARRANGE_H
#define MUSEHIP_ARRANGE_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mha_status {
  MHA_OK = 0,
  MHA_MASKED = 1,      /* valid[b] == 0 */
  MHA_BAD_COUNTS = 2,  /* n outside [0, max_notes] */
  MHA_BAD_SHIFT = 3,   /* shift[b] outside [0, 2^29] */
  MHA_MIXED = 4        /* a partner with another bpm, key or time-signature token */
};

/* notes [B, max_notes, 4], counts3 [B, 3] (notes, unused, unused), meta [B, 11]: int32, as mh_decode_events lays them out - the
 * arrays mhh_harmony_counts and mhm_structure_counts read.  valid [B], song [B], shift [B]: int32, each may be NULL (every row, one
 * song, no shift).  out_counts [B, 8] int32, out_pairs [B, 9] int64, out_ticks [B, 9] int64, status [B] int32.
 * One launch of one 256-thread block per row.  A thread keeps one of the row's notes in registers (one 16-byte load; a row of more
 * than 256 notes takes several passes), the block walks the rows of the batch, and each partner's list goes through LDS in tiles of
 * mha_key_tile() notes, shifted and with the skipped notes emptied on the way in; every thread meets its note with the tile,
 * the block folds the threads' sums with wave reductions and one thread per column stores.  Plain stores only: no global atomics,
 * no workspace, no allocation, no synchronisation (capture safe); nothing outside the output arrays is written and nothing is read
 * behind a row's counts3[., 0] notes or behind max_notes.
 * MH_ERR_INVALID, before any launch: a NULL required pointer (valid, song and shift may be NULL), B < 1, max_notes outside
 * 1..32768, B * max_notes > 2^31 (a column then stays below 2^31 * 32768 pairs of at most 65535 ticks: the int64 sums are exact). */
int mha_interplay_counts(const int32_t* notes, const int32_t* counts3, const int32_t* meta, const int32_t* valid,
                         const int32_t* song, const int32_t* shift, int32_t* out_counts, int64_t* out_pairs,
                         int64_t* out_ticks, int32_t* status, int B, int max_notes, mh_stream_t stream);

/* notes of a partner row staged through LDS per tile */
int mha_key_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_ARRANGE_H */
