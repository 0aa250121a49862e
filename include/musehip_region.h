/* musehip_region.h - region-constrained rounding of libmusehip.so / libmusehip_dbg.so (csrc/region.hip).
 *
 * An eighth header beside musehip.h, musehip_data.h, musehip_eval.h, musehip_stats.h, musehip_infill.h, musehip_harmony.h and
 * musehip_grammar.h: round the regenerated slots of an infill to whole notes.  An infill (musehip_infill.h) runs the reverse loop under
 * a mask that selects the interiors of a bar range, and mhi_infill_splice then drops what does not parse: every pad, every token of a
 * broken (position, velocity, pitch, duration) quad, every field slot whose sampled class is wrong.  With an argmax per slot one wrong
 * token costs a whole note.  The row grammar of musehip_grammar.h does not apply - every BAR, the EOS and the tail are kept tokens
 * outside the mask - but each maximal run of masked slots, a SEGMENT, obeys a grammar of four states,
 *
 *       ( PAD | POSITION VELOCITY PITCH DURATION )*
 *
 * and the best string under it is a Viterbi pass over the best token of each class at each slot: the tables of mhg_class_argmax.
 * The reference has no such step.  Everything else is shared: mh_stream_t, the mh_status return codes, enum mhg_class (the slots of
 * the tables), and the error text, which is read through mh_last_error(). */
#ifndef MUSEHIP_REGION_H
#define MUSEHIP_REGION_H

#include "musehip_grammar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tried in this order; a row that is not MHR_OK leaves as slot MHG_ANY everywhere, path_score 0 and counts 0 */
enum mhr_status {
  MHR_OK = 0,
  MHR_NOT_PLANNED = 1, /* plan_status[b] != 0: the plan has no region for the row */
  MHR_BAD_PLAN = 2,    /* field mode: a masked slot whose plan token is no position, velocity, pitch or duration */
  MHR_NONFINITE = 3,   /* a NaN or +inf score in slot PAD, PITCH, VELOCITY, DURATION or POSITION of a masked position; -inf is legal */
  MHR_NO_ROOM = 4      /* a segment without an accepted string, or (field mode) the slot to be read has no token */
};

/* cls_score / cls_idx [B * L, 8] are mhg_class_argmax's tables of the rows (or any tables of that shape); plan_tokens / plan_mask
 * [B, L] and plan_status [B] int32 are mhi_infill_plan's out_tokens / out_mask / status, fields its fields (1..15).  A slot is MASKED
 * iff plan_mask[j] == 1; any other value counts as 0.  Unmasked positions of the tables are read in slot MHG_ANY only.
 *
 * fields == 15 (whole notes).  A segment is a maximal run of masked slots.  States S (note start), V, P, D:
 *     S -> S reads PAD;  S -> V POSITION;  V -> P VELOCITY;  P -> D PITCH;  D -> S DURATION.
 *   A segment starts in S with score 0.f and must end in S.  Pads may sit anywhere between notes (the splice drops them and compacts);
 *   a quad is never interrupted, so stage (b) of the splice keeps every note placed.  Reading class c at position t adds
 *   cls_score[t, c] and emits cls_idx[t, c]; a slot whose cls_idx is negative cannot be read.  The arithmetic, which defines the
 *   result: scores step in position order with new = prev + s in plain fp32 (no contraction); reachability is kept apart from the
 *   scores, so a -inf sum is an ordinary value; into S, DURATION is listed before PAD, and PAD wins only when it is reachable and
 *   DURATION is not, or on strict > (the tie rule of mhg_constrain_rows: ties go to the note).  path_score[b] is the sum of the
 *   segments' final scores in ascending segment order, total = total + seg in fp32 from 0.f.
 * fields in 1..14.  A masked slot j emits cls_idx[j, slot] with slot the mhg_class of the infill class of plan_tokens[j] (position
 *   432..559 -> MHG_POSITION, velocity 131..194 -> MHG_VELOCITY, pitch 3..130 -> MHG_PITCH, duration 304..431 -> MHG_DURATION);
 *   path_score adds those scores in position order in the same fp32.  No automaton: the splice's class test then never rejects.
 *   NONFINITE looks at the same five slots of every masked position as whole-note mode.
 *
 * Outputs: tokens [B, L] int32 - on an MHR_OK row every masked slot holds the path's token and every other slot holds slot MHG_ANY
 * (the splice ignores those; they equal the plain argmax); status [B] int32; path_score [B] fp32; counts [B, 4] int32 = (masked
 * slots, notes placed, pads placed, segments) - notes and pads are 0 in field mode.
 * One launch of one 256-thread block per row; the mask, the segment table and one decision byte per position live in LDS, and the
 * trace-back runs in the same launch.  The status is decided before any output of the row is written.  No allocation, no workspace,
 * no atomics, no synchronisation (capture safe), plain vector stores, nothing outside the four outputs is written; the result depends
 * on the inputs alone.  MH_ERR_INVALID, before any launch: a NULL pointer, B < 1, L outside 1 .. mh_batch_max_row(), fields outside
 * 1..15. */
int mhr_constrain_regions(const float* cls_score, const int32_t* cls_idx, const int32_t* plan_tokens, const int32_t* plan_mask,
                          const int32_t* plan_status, int fields, int32_t* tokens, int32_t* status, float* path_score, int32_t* counts,
                          int B, int L, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_REGION_H */
