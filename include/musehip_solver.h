/* musehip_solver.h - the multistep DPM-Solver++ reverse step of libmusehip.so / libmusehip_dbg.so (csrc/solver.hip).
 *
 * A ninth header beside musehip.h, musehip_data.h, musehip_eval.h, musehip_stats.h, musehip_infill.h, musehip_harmony.h,
 * musehip_grammar.h and musehip_region.h: the update of DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2) for a denoiser that predicts
 * x0, as one elementwise kernel in the place of mh_ddim_epilogue / mh_step_epilogue_slots.  The reference has no such step: its short
 * loop is first-order DDIM whose update moves the latent to the level of timestep i - 1 while the next model call is made at i - gap.
 * Here the target of the step at timestep i IS the level of the next call, and the second-order term reuses the previous step's
 * prediction: one more multiply-add per element, no second model call, no noise.  Shared with musehip.h: mh_stream_t, the mh_status
 * return codes and the error text, read through mh_last_error().
 *
 * The coefficients (host, float64, rounded ONCE to fp32; models/diffusion.py GaussianDiffusion._solver_table).  With
 *   abar_t = alphas_cumprod[t], alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log(alpha_t / sigma_t)
 * and a loop that visits T - 1, T - 1 - gap, ..., the row of timestep i is
 *   target s = i - gap; s < 0 is the CLEAN level (alpha_s = 1, sigma_s = 0):              (a, b, c) = (0, 1, 0)
 *   otherwise a = sigma_s / sigma_i, e^{-h} = (sigma_s alpha_i) / (alpha_s sigma_i), phi = alpha_s (1 - e^{-h}) and
 *     order 1, or no history (i + gap > T - 1: the loop's first step):                     (a, b, c) = (a, phi, 0)
 *     order 2: h = lambda_s - lambda_i, h_prev = lambda_i - lambda_{i + gap}, r = h_prev / h:
 *                                                            (a, b, c) = (a, phi (1 + 1 / (2 r)), -phi / (2 r))
 * A row depends on i and gap alone, so a truncated loop steps with the coefficients of the full one.
 *
 * The arithmetic, which defines the result.  Per element, in fp32, every product and sum rounded on its own (no contraction):
 *     v    = x0 source: model_out[i] | table[round_idx[row]][e] | table[winner of the row's slots][e]
 *     v    = clip ? min(max(v, -1), 1) : v
 *     out  = a * x_t + b * v                      if c == 0 or x0_prev is NULL (x0_prev is NOT read: it may hold anything, NaN too)
 *     out  = (a * x_t + b * v) + c * x0_prev      otherwise
 *     out  = anchored ? x_start : out             (anchored: mask == 0, per token [rows] or per element, as in mh_ddim_epilogue)
 *     pred_xstart = v                             (at anchored positions too)
 * The slot winner is that of mh_step_epilogue_slots: over the row's nslots (pbest, pidx) pairs the larger score, on a tie the smaller
 * index - a row of -inf scores is one tie; NaN never wins, and a row of nothing else takes index 0; nslots == 0: pidx[row] is the
 * index itself.
 * Deterministic: no noise argument, the result depends on the inputs alone. */
#ifndef MUSEHIP_SOLVER_H
#define MUSEHIP_SOLVER_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one timestep's row: 32 bytes like mh_step_coef, so a [T, 8] fp32 table of these can be the coef_table of mh_step_begin /
 * mh_step_advance, which copy the current row unchanged (their pointers are then cast) */
typedef struct mhv_solver_coef {
  float a, b, c;
  float reserved[5]; /* 0 */
} mhv_solver_coef;

/* One solver step on B batch rows of per_batch = L * E elements (E = the embedding width, rows = B * per_batch / E tokens).
 * x0 source, the first that applies: pidx != NULL - the slot form: pbest / pidx [rows, nslots] with nslots > 0, or nslots == 0 and
 *   pidx [rows] (pbest is then not read); round_idx != NULL - table[round_idx[row]]; else model_out.  The first two need table [V, E].
 * coef: one row (coef_per_batch == 0) or one per batch row [B].  x0_prev: the previous step's pred_xstart, or NULL.
 * mask: NULL, [rows] (mask_per_elem == 0) or [B * per_batch] int32; it needs x_start.  pred_xstart may be NULL.
 * Aliasing: x0_prev may BE pred_xstart and out may BE x_t (the same address: every thread reads its elements before it writes
 * them); any other overlap of an output with an input or with the other output is the caller's error.
 * Two code paths with the same per-element statements and therefore the same bits: groups of 4 elements (16-byte loads and stores,
 * one coefficient / index / mask lookup per group) when E % 4 == 0 and every tensor is 16-byte aligned, else one element per thread.
 * The slot form exists in groups of 4 only.  Plain vector stores; no atomics, no workspace, no allocation, no synchronisation
 * (capture safe); nothing but out and pred_xstart is written.
 * MH_ERR_INVALID, before any launch: x_t, coef or out NULL; no x0 source; an index source without table; nslots < 0, or nslots > 0
 * without pbest; mask without x_start; B < 1, per_batch < 1, E < 1, per_batch % E != 0; the slot form with E % 4 != 0 or a tensor
 * that is not 16-byte aligned, or 2^32 or more groups of 4; more than 2^62 elements.  (The other sources run one element per thread
 * from 2^32 groups on.) */
int mhv_dpmpp_epilogue(const float* model_out, const float* x_t, const float* x0_prev, const int32_t* round_idx, const float* pbest,
                       const int32_t* pidx, int nslots, const float* table, const mhv_solver_coef* coef, int coef_per_batch, int clip,
                       const int32_t* mask, int mask_per_elem, const float* x_start, float* out, float* pred_xstart, int B,
                       int64_t per_batch, int E, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_SOLVER_H */
