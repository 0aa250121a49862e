// Region-constrained rounding (include/musehip_region.h): the masked slots of an infill plan rounded to whole notes, instead of an
// argmax per slot of which mhi_infill_splice then drops every pad, every token of a broken quad and every field slot of the wrong
// class.  Not in the reference (it has no infill).  The row grammar of grammar.hip does not apply: every BAR, the EOS and the tail are
// kept tokens outside the mask, so a row is a set of independent SEGMENTS - the maximal runs of plan_mask == 1 - and each obeys
// ( PAD | POSITION VELOCITY PITCH DURATION )*.  One kernel, one 256-thread block per row:
//   1. the mask goes to LDS (one byte per position, 1 iff plan_mask == 1) and, in the same pass, everything the status needs that one
//      position decides alone: a NaN / +inf score under the mask and, in field mode, the slot to read, its score and whether it has a token;
//   2. segment starts (mask[j] && !mask[j - 1]) get their ordinal from ballot scans over chunks of 256 positions and go to a table in LDS;
//   3. whole notes: one thread per segment, striding over the table, walks its segment serially - four states, the scores in
//      registers, the next position's 64 B of tables in flight while this one is stepped - and leaves the one real decision of a
//      position (into S: PAD instead of DURATION) as a byte in LDS; the same thread traces back and overwrites the byte with the class
//      it read.  One BYTE per position: two segments can be one slot apart (adjacent bars are), and bits packed in a word would have
//      two threads read-modify-write it;
//   4. all threads gather tokens from cls_idx, one position each, coalesced stores;
//   5. one thread adds the segment scores (field mode: the slot scores) in ascending order, which fp32 needs.
// Latency-bound integer and fp32 work on a few KiB per row: no MFMA shape here on purpose.  Conventions of infill.hip: int32 rows of
// at most mh_batch_max_row() tokens, asynchronous on the given stream, no allocation, no workspace, no atomics.
//
// Memory safety: every table index is (b L + position) 8 + slot with position < L and slot < 8 (the look-ahead load of the walk is at
// a position < L that the mask in LDS has already named); every LDS index of mask[] / dec[] / fbuf[] is a position < L <= MAX_ROW; a
// segment ordinal is below the number of segment starts, at most ceil(L / 2) <= MAX_ROW / 2 = the table's size; the status is decided
// before any output of the row is written, and every global write is inside the row's four outputs.
#include "common.h"
#include "../../include/musehip_region.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;
constexpr int MAX_ROW = 4096;      // == mh_batch_max_row() (batch.hip); the wrapper checks it

// the infill classes of infill.hip: position 0, velocity 1, pitch 2, duration 3; everything else -1
__device__ __forceinline__ int token_class(int32_t t) {
  if (t >= 432 && t <= 559) return 0;
  if (t >= 131 && t <= 194) return 1;
  if (t >= 3 && t <= 130) return 2;
  if (t >= 304 && t <= 431) return 3;
  return -1;
}

// exclusive prefix sum of one flag per thread over the block (256 threads = 4 waves); the block total to every thread
__device__ __forceinline__ int block_excl_scan(bool flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  const int before = __builtin_popcountll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __builtin_popcountll(m);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + before;
}

__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

// the five classes a region reads at one position: their scores, and bit c of `avail` set iff cls_idx[., c] >= 0
struct Slots {
  float pad, pitch, velocity, duration, position;
  unsigned avail;
};

__device__ __forceinline__ Slots load_slots(const float* __restrict__ cls_score, const int32_t* __restrict__ cls_idx, int64_t at) {
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(cls_score + at), s1 = *reinterpret_cast<const f32x4*>(cls_score + at + 4);
  const int4 i0 = *reinterpret_cast<const int4*>(cls_idx + at), i1 = *reinterpret_cast<const int4*>(cls_idx + at + 4);
  Slots r;
  r.pad = s0[MHG_PAD];
  r.pitch = s0[MHG_PITCH];
  r.velocity = s1[MHG_VELOCITY - 4];
  r.duration = s1[MHG_DURATION - 4];
  r.position = s1[MHG_POSITION - 4];
  r.avail = (i0.x >= 0 ? 1u << MHG_PAD : 0u) | (i0.w >= 0 ? 1u << MHG_PITCH : 0u) | (i1.x >= 0 ? 1u << MHG_VELOCITY : 0u) |
            (i1.y >= 0 ? 1u << MHG_DURATION : 0u) | (i1.z >= 0 ? 1u << MHG_POSITION : 0u);
  return r;
}

enum { S_S = 0, S_V = 1, S_P = 2, S_D = 3 };

__global__ __launch_bounds__(TB) void constrain_regions_kernel(const float* __restrict__ cls_score, const int32_t* __restrict__ cls_idx,
                                                              const int32_t* __restrict__ plan_tokens, const int32_t* __restrict__ plan_mask,
                                                              const int32_t* __restrict__ plan_status, int fields,
                                                              int32_t* __restrict__ tokens, int32_t* __restrict__ status,
                                                              float* __restrict__ path_score, int32_t* __restrict__ counts, int L) {
  __shared__ uint8_t mask[MAX_ROW];            // 1 iff plan_mask == 1
  __shared__ uint8_t dec[MAX_ROW];             // the walk's decision of a position, then the class the path reads there
  __shared__ uint16_t seg_start[MAX_ROW / 2];  // the first position of segment s
  __shared__ float fbuf[MAX_ROW];              // whole notes: the final score of segment s; field mode: the score read at position j
  __shared__ int wsum[4];
  __shared__ int red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t row = (int64_t)b * L;
  const bool whole = fields == 15;

  int st = plan_status[b] != 0 ? MHR_NOT_PLANNED : MHR_OK;           // uniform
  int n_masked = 0, n_seg = 0, notes = 0, pads = 0;
  float total = 0.f;
  if (st == MHR_OK) {
    // ---- 1. the mask, and what one position decides alone
    int bad_plan = 0, nonfinite = 0, no_room = 0;
    for (int j = tid; j < L; j += TB) {
      const bool mk = plan_mask[row + j] == 1;
      mask[j] = mk;
      if (!mk) continue;
      ++n_masked;
      const Slots s = load_slots(cls_score, cls_idx, (row + j) * 8);
      nonfinite |= !(s.pad < INFINITY) || !(s.pitch < INFINITY) || !(s.velocity < INFINITY) || !(s.duration < INFINITY) ||
                   !(s.position < INFINITY);                        // NaN or +inf
      if (!whole) {
        const int c = token_class(plan_tokens[row + j]);
        if (c < 0) {
          bad_plan = 1;
          continue;
        }
        const int slot = c == 0 ? MHG_POSITION : (c == 1 ? MHG_VELOCITY : (c == 2 ? MHG_PITCH : MHG_DURATION));
        dec[j] = (uint8_t)slot;
        fbuf[j] = c == 0 ? s.position : (c == 1 ? s.velocity : (c == 2 ? s.pitch : s.duration));
        no_room |= !((s.avail >> slot) & 1u);
      }
    }
    n_masked = block_sum(n_masked, red);                             // (its barriers also publish mask[], dec[] and fbuf[])
    bad_plan = block_sum(bad_plan, red);
    nonfinite = block_sum(nonfinite, red);

    // ---- 2. the segment table
    for (int j0 = 0; j0 < L; j0 += TB) {
      const int j = j0 + tid;
      const bool first = j < L && mask[j] && (j == 0 || !mask[j - 1]);
      int chunk;
      const int s = n_seg + block_excl_scan(first, wsum, chunk);
      if (first) seg_start[s] = (uint16_t)j;                         // s < ceil(L / 2)
      n_seg += chunk;
    }
    __syncthreads();

    if (bad_plan) st = MHR_BAD_PLAN;
    else if (nonfinite) st = MHR_NONFINITE;

    if (st == MHR_OK && whole) {                                     // uniform
      // ---- 3. one thread per segment: the walk, then its trace-back
      for (int s = tid; s < n_seg; s += TB) {
        const int start = seg_start[s];
        bool rS = true, rV = false, rP = false, rD = false;          // reachable, kept apart from the scores
        float sS = 0.f, sV = 0.f, sP = 0.f, sD = 0.f;
        int t = start;
        Slots cur = load_slots(cls_score, cls_idx, (row + t) * 8);
        for (;;) {
          const bool more = t + 1 < L && mask[t + 1];
          const Slots nxt = load_slots(cls_score, cls_idx, (row + (more ? t + 1 : t)) * 8);
          const bool okPAD = (cur.avail >> MHG_PAD) & 1u, okPIT = (cur.avail >> MHG_PITCH) & 1u, okVEL = (cur.avail >> MHG_VELOCITY) & 1u,
                     okDUR = (cur.avail >> MHG_DURATION) & 1u, okPOS = (cur.avail >> MHG_POSITION) & 1u;
          // into S: DURATION before PAD
          const bool b1 = rD && okDUR, b2 = rS && okPAD;
          const float f1 = sD + cur.duration, f2 = sS + cur.pad;
          const bool d = b2 && (!b1 || f2 > f1);
          const bool nrV = rS && okPOS, nrP = rV && okVEL, nrD = rP && okPIT;
          const float nV = sS + cur.position, nP = sV + cur.velocity, nD = sP + cur.pitch;
          dec[t] = d;
          rS = b1 || b2; sS = d ? f2 : f1;
          rV = nrV; sV = nV;
          rP = nrP; sP = nP;
          rD = nrD; sD = nD;
          if (!more) break;
          ++t;
          cur = nxt;
        }
        fbuf[s] = sS;
        if (!rS) {
          no_room = 1;
          continue;
        }
        int state = S_S;
        for (; t >= start; --t) {
          int c;
          if (state == S_S) {
            if (dec[t]) { c = MHG_PAD; ++pads; } else { c = MHG_DURATION; state = S_D; ++notes; }
          } else if (state == S_D) {
            c = MHG_PITCH; state = S_P;
          } else if (state == S_P) {
            c = MHG_VELOCITY; state = S_V;
          } else {
            c = MHG_POSITION; state = S_S;
          }
          dec[t] = (uint8_t)c;
        }
      }
    }
    no_room = block_sum(no_room, red);                               // (its barriers also publish dec[] and fbuf[])
    if (st == MHR_OK && no_room) st = MHR_NO_ROOM;
    notes = block_sum(notes, red);
    pads = block_sum(pads, red);

    // ---- 5. the score, added in ascending order by one thread
    if (st == MHR_OK && tid == 0) {
      if (whole) {
        for (int s = 0; s < n_seg; ++s) total = total + fbuf[s];
      } else {
        for (int j = 0; j < L; ++j)
          if (mask[j]) total = total + fbuf[j];
      }
    }
  }

  // ---- 4. the tokens: the path's class under the mask of a row that is OK, the plain argmax everywhere else
  const bool ok = st == MHR_OK;
  for (int j = tid; j < L; j += TB) {
    const int c = ok && mask[j] ? (int)dec[j] : MHG_ANY;
    tokens[row + j] = cls_idx[(row + j) * 8 + c];
  }
  if (tid == 0) {
    status[b] = st;
    path_score[b] = ok ? total : 0.f;
    counts[b * 4 + 0] = ok ? n_masked : 0;
    counts[b * 4 + 1] = ok ? notes : 0;
    counts[b * 4 + 2] = ok ? pads : 0;
    counts[b * 4 + 3] = ok ? n_seg : 0;
  }
}

}  // namespace

extern "C" int mhr_constrain_regions(const float* cls_score, const int32_t* cls_idx, const int32_t* plan_tokens, const int32_t* plan_mask,
                                     const int32_t* plan_status, int fields, int32_t* tokens, int32_t* status, float* path_score,
                                     int32_t* counts, int B, int L, mh_stream_t stream) {
  MH_CHECK_ARG(cls_score && cls_idx && plan_tokens && plan_mask && plan_status && tokens && status && path_score && counts && B > 0,
               "constrain_regions: bad arguments (a NULL pointer or B < 1)");
  MH_CHECK_ARG(L >= 1 && L <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "constrain_regions: rows of 1..%d tokens (got L = %d)", MAX_ROW, L);
  MH_CHECK_ARG(fields >= 1 && fields <= 15, "constrain_regions: fields in 1..15 (got %d)", fields);
  MH_LAUNCH(constrain_regions_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, cls_score, cls_idx, plan_tokens, plan_mask, plan_status,
            fields, tokens, status, path_score, counts, L);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
