// The multistep DPM-Solver++ reverse step (include/musehip_solver.h): x_s = a x_t + b x0 + c x0_prev on the clipped, rounded
// prediction, with the anchoring of the sampling loops - the update kernel of a loop that steps from the level of one model call to
// the level of the next, at second order from the prediction the loop already keeps.  Not in the reference.
// HBM-bound streaming: per element one or two fp32 reads beside x_t (the prediction or a table row that stays in L2, the history
// where the row has the term), two writes, three multiplies and two adds.  Two kernels with the same per-element statements
// (solver_update1, step_update.h): groups of 4 elements per thread - 16-byte loads and stores, 32-bit index math, one coefficient /
// index / mask lookup per group - for the shapes of the sampling loops, and one element per thread for everything else.
//
// Memory safety: the 4-wide kernel runs only when E % 4 == 0 and per_batch % E == 0, so a group never straddles a row, and its
// indices are 4 g .. 4 g + 3 with g < ngroups = B per_batch / 4: inside every [B, per_batch] tensor.  row = g / (E / 4) < B per_batch / E
// indexes round_idx / mask / pidx [rows]; slot reads are row nslots + sl with sl < nslots; b = g / (per_batch / 4) < B indexes coef.
// A table row comes from an index the caller vouches for (the rounding kernels emit 0 .. V - 1), as in mh_step_epilogue_slots.
// x0_prev may be pred_xstart and out may be x_t: a thread reads its own elements of both before it writes them, and no thread
// touches another's.  None of those four pointers is __restrict__.
#include "common.h"
#include "step_update.h"
#include "../../include/musehip_solver.h"

#pragma clang fp contract(off)

namespace {

constexpr int SV_BLOCK = 256;
inline int sv_grid(int64_t n_items) {
  int64_t b = (n_items + SV_BLOCK - 1) / SV_BLOCK;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));  // grid-stride beyond 8192 blocks (32 per CU)
}

enum { X0_MODEL = 0, X0_IDX = 1, X0_SLOTS = 2 };

}  // namespace

__global__ void dpmpp_epilogue_kernel(const float* __restrict__ model_out, const float* x_t, const float* x0_prev,
                                      const int32_t* __restrict__ round_idx, const float* __restrict__ table,
                                      const mhv_solver_coef* __restrict__ coef, int coef_per_batch, int clip,
                                      const int32_t* __restrict__ mask, int mask_per_elem, const float* __restrict__ x_start, float* out,
                                      float* pred_xstart, int B, int64_t per_batch, int E) {
  const int64_t total = (int64_t)B * per_batch;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / per_batch);
    const mhv_solver_coef c = coef[coef_per_batch ? b : 0];
    const bool hist = x0_prev != nullptr && c.c != 0.f;
    float x0;
    if (round_idx) x0 = table[(int64_t)round_idx[i / E] * E + (i % E)];
    else x0 = model_out[i];
    const float xt = x_t[i];
    const float prev = hist ? x0_prev[i] : 0.f;
    float sample = solver_update1(x0, xt, prev, c.a, c.b, c.c, clip, hist);
    if (mask && (mask_per_elem ? mask[i] : mask[i / E]) == 0) sample = x_start[i];
    if (pred_xstart) pred_xstart[i] = x0;
    out[i] = sample;
  }
}

// SRC: where x0 comes from (X0_MODEL / X0_IDX / X0_SLOTS).  The slot fold is step_epilogue4_kernel<*, true>'s: the larger score, on
// a tie the smaller index; nslots == 0: pidx already holds the index.
template <int SRC>
__global__ __launch_bounds__(256) void dpmpp_epilogue4_kernel(const float* __restrict__ model_out, const float* x_t, const float* x0_prev,
                                                              const int32_t* __restrict__ round_idx, const float* __restrict__ pbest,
                                                              const int32_t* __restrict__ pidx, int nslots, const float* __restrict__ table,
                                                              const mhv_solver_coef* __restrict__ coef, int coef_per_batch, int clip,
                                                              const int32_t* __restrict__ mask, int mask_per_elem,
                                                              const float* __restrict__ x_start, float* out, float* pred_xstart,
                                                              int64_t ngroups, uint32_t groups_per_batch, uint32_t groups_per_row, int E) {
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t g = (uint32_t)gi;                      // (ngroups < 2^32: checked by the launcher)
    const uint32_t b = g / groups_per_batch, row = g / groups_per_row, cg = g - row * groups_per_row;
    const mhv_solver_coef c = coef[coef_per_batch ? b : 0];
    const bool hist = x0_prev != nullptr && c.c != 0.f;
    const int64_t i = (int64_t)g * 4;
    f32x4 x0;
    if constexpr (SRC == X0_SLOTS) {
      float best = -INFINITY;
      int bi = 0x7fffffff;
      const int64_t s0 = (int64_t)row * nslots;
      if (nslots == 0) bi = pidx[row];                    // (already folded: the index itself)
      for (int sl = 0; sl < nslots; ++sl) {               // (the lanes of a row read the same addresses: one broadcast line per step)
        const float v = pbest[s0 + sl];
        const int k = pidx[s0 + sl];
        if (v > best || (v == best && k < bi)) { best = v; bi = k; }
      }
      if (bi == 0x7fffffff) bi = 0;
      x0 = *reinterpret_cast<const f32x4*>(table + (int64_t)bi * E + cg * 4);
    } else if constexpr (SRC == X0_IDX) {
      x0 = *reinterpret_cast<const f32x4*>(table + (int64_t)round_idx[row] * E + cg * 4);
    } else {
      x0 = *reinterpret_cast<const f32x4*>(model_out + i);
    }
    const f32x4 xt = *reinterpret_cast<const f32x4*>(x_t + i);
    f32x4 prev = {0.f, 0.f, 0.f, 0.f};
    if (hist) prev = *reinterpret_cast<const f32x4*>(x0_prev + i);
    f32x4 sample;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = x0[e];
      sample[e] = solver_update1(v, xt[e], prev[e], c.a, c.b, c.c, clip, hist);
      x0[e] = v;
    }
    if (mask) {
      if (mask_per_elem) {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (mask[i + e] == 0) sample[e] = x_start[i + e];
      } else if (mask[row] == 0) sample = *reinterpret_cast<const f32x4*>(x_start + i);
    }
    if (pred_xstart) *reinterpret_cast<f32x4*>(pred_xstart + i) = x0;
    *reinterpret_cast<f32x4*>(out + i) = sample;
  }
}

extern "C" int mhv_dpmpp_epilogue(const float* model_out, const float* x_t, const float* x0_prev, const int32_t* round_idx,
                                  const float* pbest, const int32_t* pidx, int nslots, const float* table, const mhv_solver_coef* coef,
                                  int coef_per_batch, int clip, const int32_t* mask, int mask_per_elem, const float* x_start, float* out,
                                  float* pred_xstart, int B, int64_t per_batch, int E, mh_stream_t stream) {
  MH_CHECK_ARG(x_t && coef && out, "dpmpp_epilogue: null pointer");
  MH_CHECK_ARG(model_out || round_idx || pidx, "dpmpp_epilogue: need model_out, round_idx or pidx");
  MH_CHECK_ARG(!(round_idx || pidx) || table, "dpmpp_epilogue: an index source needs the embedding table");
  MH_CHECK_ARG(nslots >= 0 && (!pidx || pbest || nslots == 0), "dpmpp_epilogue: nslots = %d must be >= 0, and > 0 needs pbest", nslots);
  MH_CHECK_ARG(!mask || x_start, "dpmpp_epilogue: mask needs x_start");
  MH_CHECK_ARG(B > 0 && per_batch > 0 && E > 0 && per_batch % E == 0, "dpmpp_epilogue: bad shape");
  MH_CHECK_ARG(per_batch <= (1ll << 62) / B, "dpmpp_epilogue: too many elements");
  const int src = pidx ? X0_SLOTS : (round_idx ? X0_IDX : X0_MODEL);
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // the 4-wide kernel's preconditions: whole groups per row, 16-byte aligned tensors (of those the source reads), 32-bit group numbers
  const bool groups32 = (int64_t)B * per_batch / 4 < (1ll << 32);
  const bool vec = E % 4 == 0 && groups32 && al(x_t) && al(x0_prev) && al(x_start) && al(out) && al(pred_xstart) &&
                   (src == X0_MODEL ? al(model_out) : al(table));
  MH_CHECK_ARG(src != X0_SLOTS || groups32, "dpmpp_epilogue: the slot form numbers its groups of 4 in 32 bits (got %lld)", (long long)((int64_t)B * per_batch / 4));
  MH_CHECK_ARG(src != X0_SLOTS || vec, "dpmpp_epilogue: the slot form needs E %% 4 == 0 and 16-byte aligned tensors");
  // launch note: the classes of the runtime arguments that select a path the kernel text does not show
  mh_prof_note("x0=%s mask=%s cpb=%d hist=%s fold=%d", src == X0_SLOTS ? "slots" : (src == X0_IDX ? "idx" : "model"),
               !mask ? "none" : (mask_per_elem ? "elem" : "row"), coef_per_batch != 0,
               !x0_prev ? "none" : (x0_prev == pred_xstart ? "alias" : "sep"), src == X0_SLOTS && nslots != 0);
  if (vec) {
    const int64_t ng = (int64_t)B * per_batch / 4;
    const uint32_t gpb = (uint32_t)(per_batch / 4), gpr = (uint32_t)(E / 4);
#define MHV_LAUNCH4(SRC)                                                                                                                    \
  MH_LAUNCH((dpmpp_epilogue4_kernel<SRC>), dim3(sv_grid(ng)), dim3(SV_BLOCK), 0, (hipStream_t)stream, model_out, x_t, x0_prev, round_idx, pbest, \
            pidx, nslots, table, coef, coef_per_batch, clip, mask, mask_per_elem, x_start, out, pred_xstart, ng, gpb, gpr, E)
    if (src == X0_SLOTS) MHV_LAUNCH4(X0_SLOTS);
    else if (src == X0_IDX) MHV_LAUNCH4(X0_IDX);
    else MHV_LAUNCH4(X0_MODEL);
#undef MHV_LAUNCH4
  } else {
    MH_LAUNCH(dpmpp_epilogue_kernel, dim3(sv_grid((int64_t)B * per_batch)), dim3(SV_BLOCK), 0, (hipStream_t)stream, model_out, x_t, x0_prev,
              round_idx, table, coef, coef_per_batch, clip, mask, mask_per_elem, x_start, out, pred_xstart, B, per_batch, E);
  }
  MH_CHECK_LAUNCH();
  return MH_OK;
}
