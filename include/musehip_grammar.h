/* musehip_grammar.h - grammar-constrained rounding of libmusehip.so / libmusehip_dbg.so (csrc/grammar.hip).
 *
 * A seventh header beside musehip.h, musehip_data.h, musehip_eval.h, musehip_stats.h, musehip_infill.h and musehip_harmony.h: round a
 * sampled row to the best token sequence the decoder accepts.  The sampler's last act is an argmax per position (mh_logits_argmax /
 * mh_distance_argmax); the decode path (mh_restore_chord, mh_validate_tokens, mh_decode_events) then rejects the whole row when one
 * token lands in the wrong place.  The note region of a row obeys a tiny grammar,
 *
 *       ( BAR | POSITION VELOCITY PITCH DURATION )*  EOS  PAD*          with at least one note and lo <= number of BARs <= hi,
 *
 * and the best row under it is a Viterbi pass over the best token of each class at each position.  Two launches: mhg_class_argmax
 * keeps those per-class winners of the scores the argmax kernels compute anyway, mhg_constrain_rows runs the pass and its trace-back.
 * The reference has no such step.  Everything else is shared: mh_stream_t, the mh_status return codes, and the error text, which is
 * read through mh_last_error(). */
#ifndef MUSEHIP_GRAMMAR_H
#define MUSEHIP_GRAMMAR_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the slots of the two tables: seven token classes and the whole vocabulary */
enum mhg_class {
  MHG_PAD = 0,
  MHG_EOS = 1,
  MHG_BAR = 2,
  MHG_PITCH = 3,
  MHG_VELOCITY = 4,
  MHG_DURATION = 5,
  MHG_POSITION = 6,
  MHG_ANY = 7
};

/* Seven contiguous token ranges [lo[c], hi[c]), c = MHG_PAD .. MHG_POSITION.  A host descriptor: the library reads it during the call
 * and hands it to the kernel by value - no device memory holds it.  Of a range only its part inside [0, V) counts; ranges may overlap. */
typedef struct mhg_classes {
  int32_t lo[7];
  int32_t hi[7];
} mhg_classes;

/* the ComMU vocabulary: PAD 0, EOS 1, BAR 2, PITCH 3..130, VELOCITY 131..194, DURATION 304..431, POSITION 432..559 */
int mhg_note_classes(mhg_classes* out);

/* Per token n < n_tokens and slot c: cls_score[n, c] (fp32) = the largest score of a token of class c, cls_idx[n, c] (int32) = the
 * first token that has it; slot MHG_ANY ranges over the whole vocabulary.  mode 1: score(v) = x_n . table_v + aux_v (aux = the
 * bias: mh_logits_argmax's scores); mode 2: score(v) = -sqrt(max((aux_v + |x_n|^2) - 2 x_n . table_v, 0)) (aux = |table_v|^2:
 * mh_distance_argmax's scores).  x [n_tokens, E], table [V, E], aux [V] fp32.  The same fp32 fmaf chains, expression order and tie
 * rule (strict >, first index) as those two entry points: cls_idx[n, MHG_ANY] is their answer bit for bit.  A slot starts at
 * (-inf, -1) - slot MHG_ANY at (-inf, 0), as the argmax kernels do - so a class with no token inside [0, V), or whose scores are all
 * -inf or NaN (a NaN never wins a comparison), reports (-inf, -1).  64 tokens per block, the [n_tokens, V] scores are never stored.
 * MH_ERR_INVALID: a NULL pointer, a shape below 1, a mode other than 1 or 2. */
int mhg_class_argmax(const float* x, const float* table, const float* aux, const mhg_classes* classes, float* cls_score,
                     int32_t* cls_idx, int64_t n_tokens, int E, int V, int mode, mh_stream_t stream);

enum mhg_bars {
  MHG_BARS_EXACT = 0,     /* lo = hi = n432: as many BARs as the chord part of the meta has bars */
  MHG_BARS_DECODABLE = 1  /* lo = 0, hi = n432 + 1: every count mh_restore_chord can restore */
};

/* tried in this order; a row that is not MHG_OK leaves as slot MHG_ANY everywhere, path_score 0 and counts 0 */
enum mhg_status {
  MHG_OK = 0,
  MHG_BAD_MASK = 1,          /* len_meta outside [0, L) */
  MHG_NO_CHORDS = 2,         /* n432 == 0 under a policy derived from the meta: mh_restore_chord cannot restore such a row */
  MHG_TOO_MANY_BARS = 3,     /* hi > 63 */
  MHG_BAD_BOUNDS = 4,        /* lo < 0 or lo > hi */
  MHG_NO_ROOM = 5,           /* no accepted string fits the region (it is shorter than lo + 5, or a class it needs has no token) */
  MHG_NONFINITE = 6          /* a NaN or +inf score in slots 0 .. 6 of a position of the region; -inf is legal */
};

/* The row Viterbi.  cls_score / cls_idx [B * L, 8] are mhg_class_argmax's tables of the rows (or any tables of that shape), ids /
 * mask [B, L] int32 the rows' input_ids and input_mask, bar_lo / bar_hi [B] int32 or both NULL, policy an mhg_bars.  Per row:
 *   len_meta = L - sum(mask), as mh_restore_chord computes it; n432 = the number of tokens 432 in ids[11 : len_meta - 1] (the chord
 *   part of the meta; with len_meta == 0 it ends at L - 1, as there); the note region is [len_meta, L); (lo, hi) = (bar_lo[b],
 *   bar_hi[b]) when the arrays are given, else the policy's.
 * The automaton: states A0 (event start, no note yet), B0 (event start, at least one note), V, P, D, END, times a BAR count k.
 *   A0 -> A0 (k + 1), B0 -> B0 (k + 1) read BAR;  A0 or B0 -> V reads POSITION;  V -> P VELOCITY;  P -> D PITCH;  D -> B0 DURATION;
 *   B0 -> END EOS;  END -> END PAD.   It starts in (A0, 0) and must end in END with lo <= k <= hi.
 * Reading class c at position t adds cls_score[t, c] and emits cls_idx[t, c]; a slot whose cls_idx is negative cannot be read.
 * The arithmetic, which defines the result: scores step in position order with new = prev + s in plain fp32; where two predecessors
 * meet (A0 before B0 into V, D before BAR into B0, EOS before PAD into END) the sums are compared and the later-listed one wins only
 * when it is reachable and the first is not, or on strict >; the final k is the smallest k in [lo, hi] with the maximum score.
 * Outputs: tokens [B, L] int32 = the best accepted string inside the region of a row that is MHG_OK and slot MHG_ANY everywhere
 * else (a row that cannot be constrained leaves exactly as the plain argmax leaves it); status [B]; path_score [B] fp32 = the score
 * of that string; counts [B, 3] = (BARs, notes, tokens of the region through the EOS).
 * One launch, one wave per row, the BAR count across its lanes (hence hi <= 63), the decision bits of a position as three ballot
 * words in LDS, the trace-back in the same launch.  No allocation, no synchronisation (capture safe), plain vector stores, nothing
 * outside the outputs is written.  workspace / workspace_bytes: at least mhg_constrain_workspace_bytes(B, L) bytes of device memory
 * (NULL when that is 0).  MH_ERR_INVALID, before any launch: a NULL required pointer, B < 1, L outside 1 .. mh_batch_max_row(), one
 * of bar_lo / bar_hi without the other, an unknown policy, a workspace that is too small. */
size_t mhg_constrain_workspace_bytes(int B, int L);
int mhg_constrain_rows(const float* cls_score, const int32_t* cls_idx, const int32_t* ids, const int32_t* mask, const int32_t* bar_lo,
                       const int32_t* bar_hi, int policy, int32_t* tokens, int32_t* status, float* path_score, int32_t* counts,
                       void* workspace, size_t workspace_bytes, int B, int L, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_GRAMMAR_H */
