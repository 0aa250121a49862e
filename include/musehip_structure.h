/* musehip_structure.h - the structure counts of libmusehip.so / libmusehip_dbg.so (csrc/structure.hip).
 *
 * A tenth header beside musehip.h, musehip_data.h, musehip_eval.h, musehip_stats.h, musehip_infill.h, musehip_harmony.h,
 * musehip_grammar.h, musehip_region.h and musehip_solver.h: is a decoded piece shaped like music over time?  Two statistics of the
 * MusDr set (the Jazz Transformer evaluation) that symbolic-music papers report next to the control metrics, neither of which the
 * reference computes: the pitch-class entropy of 1-bar and 4-bar windows (H1, H4) and the groove similarity of a piece's bars (GS).
 * The input is what mh_decode_events leaves on the device, the work is ragged integer work on note lists and lives here under the
 * prefix mhm_.  Everything else is shared: mh_stream_t, the mh_status return codes, and the error text, which is read through
 * mh_last_error().
 *
 * The rule, per row b with n = counts3[b, 0] notes (start tick, end tick, pitch, velocity) and meta[b, 0..10], in this order:
 *   1 time base      tpb = the ticks per bar mh_decode_events uses for meta[b, 2] (627..630: 480 * (4, 3, 3, 6) = 1920, 1440, 1440,
 *                    2880).  A slot is 120 ticks (a sixteenth note); Q = tpb / 120 = 16, 12, 12 or 24 slots a bar.
 *   2 counted notes  a note is COUNTED iff start >= 0 and k = start / tpb < max_bars and 0 <= pitch <= 127; every other note among
 *                    the row's n is SKIPPED: skipped notes are counted as such and otherwise ignored.  End tick and velocity are
 *                    not read.
 *   3 per bar        over the counted notes of bar k: n_k their number; hist_k[p], p in 0..11, those with pitch mod 12 == p; g_k,
 *                    the onset mask, with bit (start - k tpb) / 120 set for each note (bits 0..Q-1); lo_k and hi_k the lowest and
 *                    the highest pitch, -1 when the bar has no counted note.
 *   4 bars used      bars_used = 1 + the largest k over the counted notes, 0 when there is none.
 *   5 pitch use      the distinct pitches (0..127) and the distinct pitch classes of the row's counted notes.
 *   6 groove         pairs = bars_used (bars_used - 1) / 2;  diff = the sum over 0 <= j < k < bars_used of popcount(g_j xor g_k).
 *                    Bars without notes take part (g = 0).  diff <= 130816 * 24, so it fits int32.  The groove similarity of the row
 *                    is GS = 1 - diff / (Q pairs), left to the caller; it needs pairs > 0.
 *   7 entropy        for integer counts c_0..c_11 with sum N > 0:  H = (xlog2x[N] - S) / N,  S = (((xlog2x[c_0] + xlog2x[c_1]) +
 *                    xlog2x[c_2]) + ... + xlog2x[c_11]) in ascending p, every float64 add, the subtraction and the division rounded
 *                    on its own (round to nearest even, no contraction).  With xlog2x[k] = k log2 k this is the entropy in bits of
 *                    the distribution c / N.  No transcendental function is evaluated: the result is a function of the integers and
 *                    of the caller's table alone.
 *   8 windows        the 1-bar windows are the bars k < bars_used with n_k > 0; the 4-bar windows are the k = 0 .. bars_used - 4
 *                    whose four bars k .. k + 3 hold at least one counted note, with the histogram hist_k + ... + hist_{k+3}.
 *   9 outputs        out_entropy[b] = (the sum of H over the 1-bar windows, the sum over the 4-bar windows), each added in ascending
 *                    window index starting from 0.0;
 *                    out_counts[b]  = (counted, skipped, bars_used, bars with notes, pitch classes used, distinct pitches, lowest
 *                    pitch or -1, highest pitch or -1, onsets = the sum of popcount(g_k), pairs, diff, Q, 1-bar windows, 4-bar
 *                    windows, 0, 0);
 *                    bars[b, k]     = (n_k, g_k, lo_k, hi_k, hist_k[0..11]) for every k < max_bars.
 * The order of a row's notes changes no output bit. */
#ifndef MUSEHIP_STRUCTURE_H
#define MUSEHIP_STRUCTURE_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mhm_status {
  MHM_OK = 0,
  MHM_MASKED = 1,     /* valid[b] == 0 */
  MHM_BAD_META = 2,   /* key outside 602..625 or time signature outside 627..630 (the rows mhh_harmony_counts refuses) */
  MHM_BAD_COUNTS = 3  /* n outside [0, max_notes] */
};

/* notes [B, max_notes, 4], counts3 [B, 3] (notes, unused, unused), meta [B, 11], valid [B] or NULL (every row): int32, as
 * mh_decode_events lays them out - the arrays mhh_harmony_counts reads.  xlog2x [max_notes + 1]: float64, the caller's table with
 * xlog2x[0] = 0, read only at the integer counts of the rule.  out_counts [B, 16] int32, out_entropy [B, 2] float64, bars
 * [B, max_bars, 16] int32 or NULL, status [B] int32.  The statuses are tried in the order MASKED, BAD_META, BAD_COUNTS; a row that is
 * not MHM_OK gets zeros in every output (its bars table too: all sixteen fields 0) and its list is not read.
 * One launch of one 256-thread block per row: the per-bar tables live in LDS (40 KB) and are filled with LDS integer atomics, each
 * thread reads one note as 16 bytes, the windows' entropies are computed in parallel and added by one thread, the pairs of the groove
 * sum are spread over the block.  Plain stores only: no global atomics, no workspace, no allocation, no synchronisation (capture
 * safe); nothing outside the output arrays is written and nothing is read behind counts3 or the capacities.
 * MH_ERR_INVALID, before any launch: a NULL required pointer (valid and bars may be NULL), B < 1, max_notes outside 1..32768,
 * max_bars outside 1..512. */
int mhm_structure_counts(const int32_t* notes, const int32_t* counts3, const int32_t* meta, const int32_t* valid,
                         const double* xlog2x, int32_t* out_counts, double* out_entropy, int32_t* bars, int32_t* status,
                         int B, int max_notes, int max_bars, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_STRUCTURE_H */
