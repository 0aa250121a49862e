/* musehip_choose.h - choosing each song's tracks among sampled candidates, of libmusehip.so / libmusehip_dbg.so (csrc/choose.hip).
 *
 * The first header of the EXTENSION families (musediffusion_amd/_lib.py: EXTENSION_HEADERS; INTEGRATION.md, "Adding an entry-point
 * family"): its prefix has two letters, mhac_.  musehip_arrange.h says how well the rows of one song fit each other, summed over a
 * row's partners.  Here every track of a song was sampled K times, and the question is which candidate of every track to keep: that
 * needs the fit of every candidate of one track with every candidate of every OTHER track, kept apart per pair of rows
 * (mhac_pair_fit), and then a search over the combinations (mhac_choose).  Between the two stands a weighting of the interval classes
 * into one score per pair of rows, which is a few torch operations (metric.fit_scores).  Everything else is shared: mh_stream_t, the
 * mh_status return codes, the error text read through mh_last_error(), and enum mha_status.
 *
 * The layout.  A candidate batch holds S songs x T tracks x K candidates; row (s, t, k) has the index b = (s * T + t) * K + k.  So
 * B = S * T * K, a song has R = T * K rows, and a row's LOCAL index in its song is r = t * K + k.
 *
 * The rule of mhac_pair_fit, per row b with n = counts3[b, 0] notes (start tick, end tick, pitch, velocity) and s_b = shift[b] (0
 * when shift is NULL):
 *   1 in range       row c is IN RANGE iff valid[c] != 0 (every row when valid is NULL), 0 <= n_c <= max_notes and
 *                    0 <= s_c <= 2^29.
 *   2 partners       the partners of b are the rows c of b's song ON ANOTHER TRACK that are in range.  The candidates of one track
 *                    never meet.  Whether c is itself MIXED (step 3) plays no part.
 *   3 status         enum mha_status, tried in this order: MHA_MASKED (valid[b] == 0), MHA_BAD_COUNTS (n outside [0, max_notes]),
 *                    MHA_BAD_SHIFT (s_b outside [0, 2^29]), MHA_MIXED (some partner differs from b in meta[., 0], meta[., 1] or
 *                    meta[., 2]: bpm, key or time signature), MHA_OK.  A row that is not MHA_OK gets zeros in every output and its
 *                    list is not read.
 *   4 counted notes  a note is COUNTED iff 0 <= pitch <= 127 and 0 <= start < end <= 2^29; every other note among a row's n is
 *                    skipped, in b and in its partners alike.  The time of a counted note is [start + s, end + s) with its row's s;
 *                    velocity is not read.
 *   5 together       counted note x of b and counted note y of a partner SOUND TOGETHER iff
 *                    o = min(end_x, end_y) - max(start_x, start_y) > 0 in shifted times; notes that only touch do not.
 *   6 columns        a pair that sounds together, y in the partner of local index r, adds 1 to out_pairs[b, r, class] and
 *                    min(o, 65535) to out_ticks[b, r, class]; class = min(d, 12 - d) with d = |p_x - p_y| mod 12, the interval
 *                    class 0..6.  Which row lies below is not kept.
 *   7 zeros          every other [b, r, :] holds zeros, written by the kernel: r = b's own local index, a row of b's track, a row
 *                    that is not in range, and every r of a row b that is not MHA_OK.
 * Where b and the row c = s * R + r of its song are both MHA_OK, out[b, r, :] equals out[c, local(b), :]: a pair of rows is seen alike
 * from both sides.  Every output is an integer: the order of a row's notes and the launch geometry change no output bit.
 *
 * The rule of mhac_choose, per song s with the table W[s] (R x R), unary[s] (R, zeros when NULL) and eligible[s] (R, every row when
 * NULL):
 *   1 kept tracks    a track with no eligible candidate is LEFT OUT: its choice is -1 and it takes part in no term.  Every other
 *                    track is KEPT.
 *   2 combinations   a combination gives every kept track one of its candidates k_t and every left-out track k_t = 0; its index is
 *                    q = sum_t k_t K^t.  It is ADMISSIBLE iff k_t is eligible for every kept track t.
 *   3 objective      sum over the kept tracks t of unary[r_t], plus the sum over the kept tracks t < u of W[r_t, r_u], with
 *                    r_t = t * K + k_t.  Only the entry with the lower track first is read.
 *   4 outputs        best[s] = the largest objective of an admissible q; choice[s, t] = the k_t of the q that reaches it, the
 *                    smallest such q on a tie; first[s] = the objective of the smallest admissible q (candidate 0 of every track
 *                    when all of them are eligible: what one gets without choosing).  best >= first.
 *   5 status         enum mhac_status.  MHAC_BAD_SCORE iff an entry that some admissible q reads - unary[r] of an eligible r,
 *                    W[r, r'] of eligible r, r' with the track of r below the track of r' - lies outside [-2^40, 2^40]; entries
 *                    that no admissible q reads may hold anything.  With at most 210 terms the int64 sums are exact in any order.
 * The search is exact enumeration: K^T <= 2^20 (MHAC_MAX_COMBINATIONS). */
#ifndef MUSEHIP_CHOOSE_H
#define MUSEHIP_CHOOSE_H

#include "musehip_arrange.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mhac_status {
  MHAC_OK = 0,         /* every track kept */
  MHAC_PARTIAL = 1,    /* some track left out, some kept */
  MHAC_EMPTY = 2,      /* no track kept: choice -1, best 0, first 0 */
  MHAC_BAD_SCORE = 3   /* an entry that would be read lies outside +-2^40: outputs as for MHAC_EMPTY */
};

enum mhac_limit {
  MHAC_MAX_TRACKS = 20,
  MHAC_MAX_CANDIDATES = 16,
  MHAC_MAX_COMBINATIONS = 1048576   /* 2^20 */
};

/* notes [B, max_notes, 4], counts3 [B, 3] (notes, unused, unused), meta [B, 11]: int32, as mh_decode_events lays them out.
 * valid [B], shift [B]: int32, each may be NULL (every row, no shift).  out_ticks [B, R, 7] and out_pairs [B, R, 7] int64,
 * status [B] int32 (enum mha_status).
 * One launch of one 256-thread block per row.  A thread keeps one of the row's notes in registers, the block walks the R rows of its
 * song, and each partner's list goes through LDS in tiles of mhac_key_tile() notes, shifted and with the skipped notes emptied on the
 * way in; every thread meets its note with the tile, and PER PARTNER the block folds the threads' sums with wave reductions and one
 * thread per column stores.  Plain stores only: no global atomics, no workspace, no allocation, no synchronisation (capture safe);
 * every output element is written, nothing outside the output arrays is, and nothing is read behind a row's counts3[., 0] notes or
 * behind max_notes.
 * MH_ERR_INVALID, before any launch: a NULL required pointer (valid and shift may be NULL), S < 1, T outside 1..20, K outside 1..16,
 * max_notes outside 1..32768, B * max_notes > 2^31 or B >= 2^31. */
int mhac_pair_fit(const int32_t* notes, const int32_t* counts3, const int32_t* meta, const int32_t* valid, const int32_t* shift,
                  int64_t* out_ticks, int64_t* out_pairs, int32_t* status, int S, int T, int K, int max_notes, mh_stream_t stream);

/* notes of a partner row staged through LDS per tile */
int mhac_key_tile(void);

/* W [S, R, R] int64; unary [S, R] int64, may be NULL (zeros); eligible [S, R] int32, may be NULL (every row).  choice [S, T] int32,
 * best [S] and first [S] int64, status [S] int32 (enum mhac_status).
 * One launch of one 256-thread block per song.  The block brings the song's table into LDS (R <= 80 under the limit below: 50 KiB),
 * lists every kept track's eligible candidates, and its threads walk the admissible combinations in the order of q, a thread adding
 * a combination's terms from LDS; the block folds (objective, q) pairs with wave reductions.  No workspace, no allocation, no
 * synchronisation (capture safe); nothing outside the outputs is written.
 * MH_ERR_INVALID, before any launch: a NULL required pointer (unary and eligible may be NULL), S < 1, T outside 1..20, K outside
 * 1..16.  MH_ERR_UNSUPPORTED: K^T > 2^20 - the search is exact; approximate search beyond the limit is not built. */
int mhac_choose(const int64_t* W, const int64_t* unary, const int32_t* eligible, int32_t* choice, int64_t* best, int64_t* first,
                int32_t* status, int S, int T, int K, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_CHOOSE_H */
