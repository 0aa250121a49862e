/* musehip_eval.h - the evaluation entry points of libmusehip.so / libmusehip_dbg.so (csrc/evaluate.hip).
 *
 * A third header beside musehip.h and musehip_data.h: the evaluation end of a sampling run (MuseDiffusion/run/sample.py:245-273,
 * MuseDiffusion/metric.py:83-117) lives here under the prefix mhe_.  Everything else is shared: mh_stream_t, the mh_status return
 * codes, and the error text, which is read through mh_last_error(). */
#ifndef MUSEHIP_EVAL_H
#define MUSEHIP_EVAL_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fused 1-nearest-neighbour search under the MSIM similarity: for every query row the most similar key row, without writing the
 * similarity matrix.  q [nq, 56] and k [nk, 56] are fp32 rows as mh_msim_vectors writes them (32 rhythm, 12 melody, 12 harmony):
 *   sim(i, j) = (dot32(q_i[0:32], k_j[0:32]) * dot12(q_i[32:44], k_j[32:44])) * dot12(q_i[44:56], k_j[44:56])
 * each dot one fmaf chain over ascending element index that starts from 0, the two multiplies plain fp32: metric.py:100-103 in the
 * reference's operand order.  The operations of a pair (i, j) do not depend on the launch geometry or on j's place in a tile: equal
 * key rows give bit-equal similarities.
 *   self = 1        q and k are the same set (q == k, nq == nk, q_valid == k_valid): sim(i, i) is replaced by 0.0f, which takes part
 *                   in the maximum (metric.py:104, fill_diagonal_(0)).
 *   selection       torch.argmax's rule: the largest value, the lowest j among equal values; a NaN beats every number and the first
 *                   NaN wins.  A key row with k_valid[j] == 0 is skipped; a query row with q_valid[i] == 0, or with no candidate, gets
 *                   most[i] = -1 and best[i] = 0.  Indices are into the arrays as given (nothing is compacted).
 *   q_valid, k_valid  int32 [nq] / [nk], NULL = every row valid.
 *   most, best      int32 / fp32 [nq]; best may be NULL.
 *   sim             NULL, or fp32 [nq, nk] (tests, small sets): sim(i, j) of every valid query row i and valid key row j, the diagonal
 *                   as selected from; the entries of masked rows and columns are left as they are.
 * Deterministic (no atomics); one launch; nothing is read or written outside the buffers for any validity pattern.
 * MH_ERR_INVALID: a NULL q / k / most, nq or nk outside 1..2^31 / 56, self = 1 with q != k, nq != nk or q_valid != k_valid. */
int mhe_msim_nearest(const float* q, int64_t nq, const float* k, int64_t nk, const int32_t* q_valid, const int32_t* k_valid, int self,
                     int32_t* most, float* best, float* sim, mh_stream_t stream);
/* Rows of k staged through LDS per tile.  Each of the block's four waves takes a quarter of a tile, and a wave walks its quarter in
 * 1, 2 or 4 slices (chosen from nq: fewer query rows per block when the query set is small, so that it still spreads over the
 * chip).  The places where a key's handling changes hands (tests put duplicated rows on both sides of them): multiples of this, of
 * a quarter and of a sixteenth of it. */
int mhe_nearest_key_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_EVAL_H */
