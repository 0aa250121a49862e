/* musehip_infill.h - the infill entry points of libmusehip.so / libmusehip_dbg.so (csrc/infill.hip).
 *
 * A fifth header beside musehip.h, musehip_data.h, musehip_eval.h and musehip_stats.h: "keep the piece, regenerate bars lo..hi" and
 * "keep the rhythm, regenerate the pitches" are a mask that follows the token grammar on the way into the reverse loop and a splice on
 * the way out of it.  Both are ragged integer work on [B, L] token rows and live here under the prefix mhi_.  Everything else is
 * shared: mh_stream_t, the mh_status return codes, and the error text, which is read through mh_last_error().
 *
 * Grammar of a row: a prefix (meta and chord tokens, prefix_mask == 0), then BAR (2), (position, velocity, pitch, duration) quads,
 * ..., EOS (1), then a tail.  Token classes: position 432..559 = 0, velocity 131..194 = 1, pitch 3..130 = 2, duration 304..431 = 3,
 * every other int32 (pad 0, EOS, BAR, chord and meta tokens, negatives, anything above 559) = -1.
 *
 * Per row:  m   = the number of leading tokens with prefix_mask == 0
 *           e   = the first index >= m holding EOS
 *           p_0 < ... < p_{nb-1} = the indices in [m, e) holding BAR, p_nb := e
 *           the INTERIOR of bar k = the indices j with p_k < j < p_{k+1}
 *           the selected bars = lo <= k < hi (bar_lo[b], bar_hi[b]).
 * BAR tokens, tokens before p_0, EOS and the tail are never selected. */
#ifndef MUSEHIP_INFILL_H
#define MUSEHIP_INFILL_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mhi_status {
  MHI_OK = 0,
  MHI_NO_EOS = 1,    /* no EOS at or behind index m */
  MHI_BAD_MASK = 2,  /* prefix_mask is not m zeros followed by L - m ones with 0 < m < L */
  MHI_BAD_RANGE = 3, /* not 0 <= lo < hi <= nb */
  MHI_OVERFLOW = 4   /* e + 1 + added > L: the widened row would lose its EOS */
};

/* The mask of an infill and the row it applies to.  All arrays are int32; tokens / prefix_mask / out_tokens / out_mask are [B, L]
 * row-major, bar_lo / bar_hi / status [B], info [B, 4].  The statuses are tried in the order BAD_MASK, NO_EOS, BAD_RANGE, OVERFLOW.
 * A row that is not MHI_OK: out_tokens = tokens, out_mask = 0, info = 0 (a reverse loop under that mask returns the row as it is).
 *   fields == 15 (whole notes)  behind the interior of every selected bar g = 4 room pad (0) slots are inserted; added = g (hi - lo).
 *       out_tokens is the row with the insertions, cut at L: the tail behind EOS moves right and its last `added` tokens fall off.
 *       out_mask is 1 on every interior slot of a selected bar, old and inserted, 0 elsewhere.
 *   fields in 1..14 (bit 0 position, 1 velocity, 2 pitch, 3 duration; room must be 0)  out_tokens = tokens; out_mask[j] = 1 iff j lies
 *       in a selected interior, c = class(tokens[j]) >= 0, the four tokens at q = j - c .. q + 3 all lie in that same interior with
 *       the classes 0, 1, 2, 3, and bit c of fields is set.
 *   info[b] = (p_lo + 1: the first region slot; one past the last region slot in out_tokens = p_hi + added; the number of
 *       out_mask == 1 slots; added).
 * One launch of one 256-thread block per row; the row is staged in LDS and the status is decided before anything is written.  No
 * atomics, no workspace, no allocation, no synchronisation (capture safe); nothing is read or written outside [B, L] for any input.
 * MH_ERR_INVALID, before any launch: a NULL pointer, B < 1, L outside 1..mh_batch_max_row(), room < 0, fields outside 1..15,
 * fields != 15 with room != 0. */
int mhi_infill_plan(const int32_t* tokens, const int32_t* prefix_mask, const int32_t* bar_lo, const int32_t* bar_hi, int room, int fields,
                    int32_t* out_tokens, int32_t* out_mask, int32_t* status, int32_t* info, int B, int L, mh_stream_t stream);

/* The way back: sampled [B, L] are the tokens a reverse loop returned for (plan_tokens, plan_mask), status [B] the plan's.
 * out [B, L], counts [B, 4], all int32.
 *   a row whose status is not MHI_OK   out = plan_tokens, counts = 0.
 *   a slot with plan_mask == 0         takes plan_tokens[j]; sampled[j] is not looked at.
 *   fields in 1..14   a plan_mask == 1 slot takes sampled[j] if class(sampled[j]) == class(plan_tokens[j]), else plan_tokens[j]
 *                     (counted as rejected).  Nothing moves.
 *   fields == 15      two stages.  (a) the plan_mask == 1 slots whose sampled token is 0 (counted as pads) or of class -1 (counted as
 *                     other) are dropped and the row is compacted.  (b) in the compacted row a region token (one that came from a
 *                     plan_mask == 1 slot) of class c at index i survives iff the four tokens at i - c .. i - c + 3 are all region
 *                     tokens with the classes 0, 1, 2, 3; the others are counted as other.  The row is compacted again and filled to L
 *                     with pad 0.  An anchored BAR has class -1 and is no region token, so no quad straddles a bar.
 *   counts[b] = (region tokens kept, pads dropped, other dropped or rejected, kept region slots whose token differs from plan_tokens
 *                at that slot - field mode only, 0 for fields == 15).  For fields == 15 kept % 4 == 0 and kept + pads + other is
 *                the plan's info[2].
 * One launch of one 256-thread block per row, as mhi_infill_plan.  MH_ERR_INVALID: a NULL pointer, B < 1, L outside
 * 1..mh_batch_max_row(), fields outside 1..15. */
int mhi_infill_splice(const int32_t* sampled, const int32_t* plan_tokens, const int32_t* plan_mask, const int32_t* status, int fields,
                      int32_t* out, int32_t* counts, int B, int L, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_INFILL_H */
