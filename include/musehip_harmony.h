/* musehip_harmony.h - the chord-fit counts of libmusehip.so / libmusehip_dbg.so (csrc/harmony.hip).
 *
 * A sixth header beside musehip.h, musehip_data.h, musehip_eval.h, musehip_stats.h and musehip_infill.h: do the notes of a decoded
 * piece fit the chord progression the piece was conditioned on?  That is CH, the third control metric of the ComMU paper next to CP
 * and CV; the reference has no code for it.  The input is what mh_decode_events leaves on the device, the work is ragged integer work
 * on note and chord lists and lives here under the prefix mhh_.  Everything else is shared: mh_stream_t, the mh_status return codes,
 * and the error text, which is read through mh_last_error().
 *
 * The rule, per row b with n = counts3[b, 0] notes (start tick, end tick, pitch, velocity), c = counts3[b, 1] chord changes
 * (tick, chord token) and meta[b, 0..10].  All of it is integer arithmetic:
 *   time base    tpb = the ticks per bar mh_decode_events uses for meta[b, 2] (627..630: 1920, 1440, 1440, 2880).  The key token
 *                k = meta[b, 1] is 602..625; the tonic pitch class is (k - 602) mod 12 and the key is minor iff k >= 614.
 *   pitch class  pc = pitch mod 12, non-negative for any int32 pitch.
 *   chord in force at a note   of the entries j < c with tick_j <= start (signed) the one with the largest tick; among equal ticks
 *                the last in list order; none qualifies: no chord is in force.  A chord exactly at the start is in force.  The list
 *                need not be sorted and the answer does not depend on whether it is.  THE CHORD AT THE ONSET JUDGES THE WHOLE NOTE: a
 *                note that sounds across a chord change is not split.
 *   chord tones  a chord token is 195 + 9 r + q, r in 0..11 (roots a, a#, b, c, ..., g#: root pitch class (9 + r) mod 12), q in 0..8:
 *                "" {0,4,7}  "7" {0,4,7,10}  "+" {0,4,8}  "dim" {0,3,6}  "m" {0,3,7}  "m7" {0,3,7,10}  "m7b5" {0,3,6,10}
 *                "maj7" {0,4,7,11}  "sus4" {0,5,7} over the root.  Token 303 (NN) and any token outside 195..302 name no chord.  A
 *                note is JUDGED iff a chord is in force and names one; a judged note is a CHORD TONE iff its pc is in the set.
 *   scale tones  major {0,2,4,5,7,9,11}, natural minor {0,2,3,5,7,8,10} over the tonic; every note is tested, judged or not.
 *   length       min(max(end - start, 0), 65535) ticks, so that with max_notes <= 32768 no sum leaves int32.
 *
 * Known limitation: the encoder's vocabulary folds eighteen chord types into these nine ("6" becomes major, "sus2" and "add2" become
 * "maj7", "dim7" becomes "dim", "m6" becomes "m", "madd2" and "mM7" become "m7", "7sus4" becomes "sus4").  The counts judge against
 * the chord the model was conditioned on, not the chord the arranger wrote: the sixth of a "6" chord counts as off. */
#ifndef MUSEHIP_HARMONY_H
#define MUSEHIP_HARMONY_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mhh_status {
  MHH_OK = 0,
  MHH_MASKED = 1,     /* valid[b] == 0 */
  MHH_BAD_META = 2,   /* key outside 602..625 or time signature outside 627..630 */
  MHH_BAD_COUNTS = 3  /* n outside [0, max_notes] or c outside [0, max_chords] */
};

/* All arrays are int32: notes [B, max_notes, 4], chords [B, max_chords, 2], counts3 [B, 3] (notes, chords, unused), meta [B, 11],
 * valid [B] or NULL (every row), as mh_decode_events lays them out; out_counts [B, 8], hist [B, 12] or NULL, bars [B, max_bars, 4]
 * or NULL, status [B].  The statuses are tried in the order MASKED, BAD_META, BAD_COUNTS; a row that is not MHH_OK gets zeros in every
 * output and its lists are not read.
 *   out_counts[b] = (notes, judged, chord tones, scale tones, ticks of all notes, ticks of judged notes, ticks of chord tones,
 *                    bars_used = 1 + the largest start / tpb over the notes with start >= 0, or 0 when there is none)
 *   hist[b, p]    = the notes of pitch class p
 *   bars[b, k]    = (notes, judged, chord tones, scale tones) of the notes that start in bar k = start / tpb.  Only notes with
 *                   start >= 0 and k < max_bars go in (they all count in out_counts; bars_used > max_bars tells the caller); a bar
 *                   without notes is zero.
 * One launch of one 256-thread block per row: the chord list is staged in LDS, each thread reads one note as 16 bytes, a sorted chord
 * list is searched by bisection and an unsorted one scanned.  Plain stores only: no global atomics, no workspace, no allocation, no
 * synchronisation (capture safe); nothing outside the output arrays is written and nothing is read behind counts3 or the capacities.
 * MH_ERR_INVALID, before any launch: a NULL required pointer, B < 1, max_notes outside 1..32768, max_chords outside 1..4096,
 * max_bars outside 0..512, bars without max_bars or max_bars without bars. */
int mhh_harmony_counts(const int32_t* notes, const int32_t* chords, const int32_t* counts3, const int32_t* meta, const int32_t* valid,
                       int32_t* out_counts, int32_t* hist, int32_t* bars, int32_t* status, int B, int max_notes, int max_chords,
                       int max_bars, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_HARMONY_H */
