/* musehip_stats.h - the set-statistics entry points of libmusehip.so / libmusehip_dbg.so (csrc/pairstats.hip).
 *
 * A fourth header beside musehip.h, musehip_data.h and musehip_eval.h: what a run can say about a set of pieces WITHOUT a ground truth
 * (how different its members are from each other, how many are the same piece twice) rests on a sum and on counts over all pairs of
 * the set under the MSIM similarity.  Those reductions live here under the prefix mhs_.  Everything else is shared: mh_stream_t, the
 * mh_status return codes, and the error text, which is read through mh_last_error(). */
#ifndef MUSEHIP_STATS_H
#define MUSEHIP_STATS_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pair statistics under the MSIM similarity: per query row a sum and three counts over its counted pairs, without writing the
 * similarity matrix.  q [nq, 56] and k [nk, 56] are fp32 rows as mh_msim_vectors writes them; sim(i, j) is the value of
 * mhe_msim_nearest (musehip_eval.h) bit for bit - one device function serves both - whatever the launch geometry.
 *   counted pairs   for query row i the pairs (i, j) with k_valid[j] != 0, q_group[i] == k_group[j], and j != i when self = 1.
 *   self = 1        q and k are the same set (q == k, nq == nk, q_valid == k_valid, q_group == k_group).  A row is not a pair with
 *                   itself: the diagonal touches none of the outputs (mhe_msim_nearest lets it take part as 0; not so here).
 *   q_valid, k_valid  int32 [nq] / [nk], NULL = every row valid.
 *   q_group, k_group  int32 [nq] / [nk] group ids, NULL = one group (id 0 on that side).  Any int32 is an ordinary id.
 *   nan[i]          int32: the counted pairs whose similarity is NaN (a row without notes carries a 0 / 0 harmony vector).
 *   count[i]        int32: the counted pairs whose similarity is not NaN.
 *   sum[i]          float64: the sum of the fp32 similarities of those count[i] pairs, accumulated in float64.
 *   above[i]        int32, may be NULL: how many of those count[i] pairs have sim >= threshold, compared in fp32.  A NaN threshold
 *                   counts nothing.
 * A query row with q_valid[i] == 0, or without a counted pair, gets 0 / 0 / 0 / 0.0.
 * Order: a lane adds its keys in ascending j, a row's partial sums are added in ascending order of the key slices: the same call gives
 * the same bits.  Another geometry (nq decides how many slices share a row) partitions the same terms differently; the float64
 * accumulation keeps that within 2 (count - 1) 2^-53 sum |sim|.  The integers do not depend on the geometry.
 * No atomics, no workspace; one launch; nothing is read or written outside the buffers for any mask or group pattern.
 * MH_ERR_INVALID: a NULL q / k / sum / count / nan, nq or nk outside 1..2^31 / 56, self outside {0, 1}, self = 1 with q != k,
 * nq != nk, q_valid != k_valid or q_group != k_group. */
int mhs_msim_pair_stats(const float* q, int64_t nq, const float* k, int64_t nk, const int32_t* q_valid, const int32_t* k_valid,
                        const int32_t* q_group, const int32_t* k_group, int self, float threshold, double* sum, int32_t* count,
                        int32_t* nan, int32_t* above, mh_stream_t stream);
/* Rows of k staged through LDS per tile; as mhe_nearest_key_tile(): a key's handling changes hands at multiples of this, of a quarter
 * and of a sixteenth of it. */
int mhs_pair_key_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_STATS_H */
