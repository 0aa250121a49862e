// The MSIM similarity of one (query, key) pair, shared by every kernel that judges pairs (evaluate.hip: the nearest neighbour;
// pairstats.hip: the pair statistics), so that a pair has one value - the same bits - whichever kernel, wave, slice, tile slot or grid
// handles it.  Rows are [32 rhythm | 12 melody | 12 harmony] fp32 as mh_msim_vectors writes them.
#pragma once

#pragma clang fp contract(off)

namespace msim {

constexpr int DR = 32, DM = 12, DH = 12, D = DR + DM + DH;

// the operation order include/musehip_eval.h states: three fmaf chains over ascending element index from 0, then (r * m) * h
__device__ __forceinline__ float msim_pair(const float (&qv)[D], const float* __restrict__ kr) {
  float r = 0.0f, m = 0.0f, h = 0.0f;
#pragma unroll
  for (int e = 0; e < DR; ++e) r = __builtin_fmaf(qv[e], kr[e], r);
#pragma unroll
  for (int e = 0; e < DM; ++e) m = __builtin_fmaf(qv[DR + e], kr[DR + e], m);
#pragma unroll
  for (int e = 0; e < DH; ++e) h = __builtin_fmaf(qv[DR + DM + e], kr[DR + DM + e], h);
  return (r * m) * h;
}

}  // namespace msim
