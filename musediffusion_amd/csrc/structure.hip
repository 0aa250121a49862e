// Structure counts on the device (include/musehip_structure.h): for every decoded row the per-bar note counts, pitch-class histograms,
// onset masks and pitch ranges, from them the sums of the pitch-class entropy over 1-bar and 4-bar windows (H1, H4 of the MusDr set)
// and the pairwise onset-mask distance of the bars (groove similarity, GS).  Not in the reference: it reports nothing over time.  The
// input is what decode_events_kernel (decode.hip) writes.  Conventions of harmony.hip: one 256-thread block per row, the per-bar
// tables in LDS, int32 in, asynchronous on the given stream, no allocation.  Latency-bound integer work - no MFMA shape here.
//
// Bit-for-bit by construction: the tables are filled with LDS integer atomics (add, or, min, max), which do not depend on the order
// of the notes; an entropy is xlog2x[] entries of the caller's table added in a fixed order, one subtraction and one division, each
// rounded on its own (the _rn intrinsics, contraction off for the file), and ONE thread adds the windows in ascending index.
//
// Memory safety: n <= max_notes is part of the status, decided before the list is touched; a counted note has 0 <= k < max_bars <=
// MAX_BARS, 0 <= pitch <= 127 and a slot below Q <= 24, so every LDS index is inside its table; a histogram sums to at most n <=
// max_notes, the last entry of xlog2x; every global index is inside its row.
#include "common.h"
#include "../../include/musehip_structure.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;
constexpr int MAX_NOTES = 32768, MAX_BARS = 512;
constexpr int NO_PITCH = 128;                                          // above every counted pitch: the empty bar's lo before it is read

// row totals in LDS, one integer atomic per wave and field
enum { T_COUNTED, T_WITH, T_ONSETS, T_TOP, T_LO, T_HI, T_PCS, T_W4, T_DIFF, T_N };

// H = (xlog2x[N] - S) / N over twelve counts, S added in ascending pitch class from the first entry (the header's step 7)
__device__ __forceinline__ double entropy12(const int (&c)[12], int N, const double* __restrict__ xlog2x) {
  double S = __dadd_rn(xlog2x[c[0]], xlog2x[c[1]]);
#pragma unroll
  for (int p = 2; p < 12; ++p) S = __dadd_rn(S, xlog2x[c[p]]);
  return __ddiv_rn(__dsub_rn(xlog2x[N], S), (double)N);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ int wave_min(int v) { return -wave_max(-v); }   // |v| <= 128 here

__global__ __launch_bounds__(TB) void structure_counts_kernel(const int32_t* __restrict__ notes, const int32_t* __restrict__ counts3,
                                                             const int32_t* __restrict__ meta, const int32_t* __restrict__ valid,
                                                             const double* __restrict__ xlog2x, int32_t* __restrict__ out_counts,
                                                             double* __restrict__ out_entropy, int32_t* __restrict__ bars,
                                                             int32_t* __restrict__ status, int max_notes, int max_bars) {
  __shared__ int s_n[MAX_BARS];
  __shared__ unsigned s_g[MAX_BARS];
  __shared__ int s_lo[MAX_BARS];
  __shared__ int s_hi[MAX_BARS];
  __shared__ int s_hist[MAX_BARS * 12];
  __shared__ double s_h1[MAX_BARS];
  __shared__ double s_h4[MAX_BARS];
  __shared__ unsigned s_pitch[4];                                      // the 128-bit mask of the pitches used
  __shared__ int s_tot[T_N];
  const int b = blockIdx.x, tid = threadIdx.x;
  int32_t* obars = bars ? bars + (int64_t)b * max_bars * 16 : nullptr;

  // ---- the status: one word per block, decided before anything is written and before the list is read
  int st = MHM_OK, n = 0, tpb = 1920;
  if (valid && valid[b] == 0) {
    st = MHM_MASKED;
  } else {
    const int32_t key = meta[b * 11 + 1], ts = meta[b * 11 + 2];
    if (!(key >= 602 && key <= 625 && ts >= 627 && ts <= 630)) {
      st = MHM_BAD_META;
    } else {
      n = counts3[b * 3 + 0];
      if (n < 0 || n > max_notes) st = MHM_BAD_COUNTS;
      tpb = 480 * (ts == 627 ? 4 : (ts == 630 ? 6 : 3));              // decode_events_kernel's beats per bar
    }
  }
  if (st != MHM_OK) {                                                  // uniform
    if (tid < 16) out_counts[b * 16 + tid] = 0;
    if (tid < 2) out_entropy[b * 2 + tid] = 0.0;
    if (obars)
      for (int i = tid; i < max_bars * 16; i += TB) obars[i] = 0;
    if (tid == 0) status[b] = st;
    return;
  }

  // ---- empty tables
  for (int k = tid; k < max_bars; k += TB) {
    s_n[k] = 0;
    s_g[k] = 0u;
    s_lo[k] = NO_PITCH;
    s_hi[k] = -1;
  }
  for (int i = tid; i < max_bars * 12; i += TB) s_hist[i] = 0;
  if (tid < 4) s_pitch[tid] = 0u;
  if (tid < T_N) s_tot[tid] = tid == T_TOP || tid == T_HI ? -1 : (tid == T_LO ? NO_PITCH : 0);
  __syncthreads();

  // ---- one note per thread and pass; integer atomics: the order of the notes does not matter
  const int32_t* nrow = notes + (int64_t)b * max_notes * 4;
  for (int j = tid; j < n; j += TB) {
    int32_t v[4];
    __builtin_memcpy(v, nrow + 4 * (int64_t)j, 16);                    // the whole note (harmony.hip); the compiler keeps the two words used
    const int32_t start = v[0], pitch = v[2];
    if (start < 0 || pitch < 0 || pitch > 127) continue;
    const int k = start / tpb;
    if (k >= max_bars) continue;
    const int slot = (start - k * tpb) / 120;                          // below Q = tpb / 120 <= 24
    atomicAdd(&s_n[k], 1);
    atomicAdd(&s_hist[k * 12 + pitch % 12], 1);
    atomicOr(&s_g[k], 1u << slot);
    atomicMin(&s_lo[k], pitch);
    atomicMax(&s_hi[k], pitch);
    atomicOr(&s_pitch[pitch >> 5], 1u << (pitch & 31));
  }
  __syncthreads();

  // ---- one bar per thread and pass: the row totals, the 1-bar windows, lo = -1 for the bars without notes
  {
    int counted = 0, with = 0, onsets = 0, top = -1, lo = NO_PITCH, hi = -1;
    for (int k = tid; k < max_bars; k += TB) {
      const int nk = s_n[k];
      if (nk > 0) {
        counted += nk;
        with += 1;
        onsets += __builtin_popcount(s_g[k]);
        top = k;                                                       // k ascends
        lo = s_lo[k] < lo ? s_lo[k] : lo;
        hi = s_hi[k] > hi ? s_hi[k] : hi;
        int c[12];
#pragma unroll
        for (int p = 0; p < 12; ++p) c[p] = s_hist[k * 12 + p];
        s_h1[k] = entropy12(c, nk, xlog2x);
      } else {
        s_lo[k] = -1;
      }
    }
    counted = wave_sum(counted); with = wave_sum(with); onsets = wave_sum(onsets);
    top = wave_max(top); lo = wave_min(lo); hi = wave_max(hi);
    if ((tid & 63) == 0) {
      atomicAdd(&s_tot[T_COUNTED], counted);
      atomicAdd(&s_tot[T_WITH], with);
      atomicAdd(&s_tot[T_ONSETS], onsets);
      atomicMax(&s_tot[T_TOP], top);
      atomicMin(&s_tot[T_LO], lo);
      atomicMax(&s_tot[T_HI], hi);
    }
    if (tid < 128 && ((s_pitch[tid >> 5] >> (tid & 31)) & 1u)) atomicOr(&s_tot[T_PCS], 1 << (tid % 12));
  }
  __syncthreads();
  const int used = s_tot[T_TOP] + 1;                                   // bars_used <= max_bars

  // ---- the 4-bar windows k = 0 .. used - 4
  {
    int w4 = 0;
    for (int k = tid; k + 4 <= used; k += TB) {
      const int N = s_n[k] + s_n[k + 1] + s_n[k + 2] + s_n[k + 3];
      if (N > 0) {
        int c[12];
#pragma unroll
        for (int p = 0; p < 12; ++p) c[p] = s_hist[k * 12 + p] + s_hist[(k + 1) * 12 + p] + s_hist[(k + 2) * 12 + p] + s_hist[(k + 3) * 12 + p];
        s_h4[k] = entropy12(c, N, xlog2x);
        w4 += 1;
      }
    }
    w4 = wave_sum(w4);
    if ((tid & 63) == 0) atomicAdd(&s_tot[T_W4], w4);
  }
  __syncthreads();

  // ---- one thread adds the windows in ascending index (512 terms each at most) while the block takes the pairs
  if (tid == TB - 1) {
    double h1 = 0.0, h4 = 0.0;
    for (int k = 0; k < used; ++k)
      if (s_n[k] > 0) h1 = __dadd_rn(h1, s_h1[k]);
    for (int k = 0; k + 4 <= used; ++k)
      if (s_n[k] + s_n[k + 1] + s_n[k + 2] + s_n[k + 3] > 0) h4 = __dadd_rn(h4, s_h4[k]);
    out_entropy[b * 2 + 0] = h1;
    out_entropy[b * 2 + 1] = h4;
  }
  {
    // rows j and used - 1 - j of the upper triangle together hold used - 1 pairs: the same work for every r
    int diff = 0;
    for (int r = tid; 2 * r < used; r += TB) {
      const int j2 = used - 1 - r;
      const unsigned g = s_g[r];
      for (int k = r + 1; k < used; ++k) diff += __builtin_popcount(g ^ s_g[k]);
      if (j2 != r) {
        const unsigned g2 = s_g[j2];
        for (int k = j2 + 1; k < used; ++k) diff += __builtin_popcount(g2 ^ s_g[k]);
      }
    }
    diff = wave_sum(diff);
    if ((tid & 63) == 0) atomicAdd(&s_tot[T_DIFF], diff);
  }
  if (obars)
    for (int i = tid; i < max_bars * 16; i += TB) {
      const int k = i >> 4, f = i & 15;
      obars[i] = f == 0 ? s_n[k] : (f == 1 ? (int)s_g[k] : (f == 2 ? s_lo[k] : (f == 3 ? s_hi[k] : s_hist[k * 12 + f - 4])));
    }
  __syncthreads();

  if (tid == 0) {
    const int counted = s_tot[T_COUNTED];
    int32_t* o = out_counts + b * 16;
    o[0] = counted;
    o[1] = n - counted;
    o[2] = used;
    o[3] = s_tot[T_WITH];
    o[4] = __builtin_popcount((unsigned)s_tot[T_PCS]);
    o[5] = __builtin_popcount(s_pitch[0]) + __builtin_popcount(s_pitch[1]) + __builtin_popcount(s_pitch[2]) + __builtin_popcount(s_pitch[3]);
    o[6] = counted ? s_tot[T_LO] : -1;
    o[7] = s_tot[T_HI];
    o[8] = s_tot[T_ONSETS];
    o[9] = used * (used - 1) / 2;
    o[10] = s_tot[T_DIFF];
    o[11] = tpb / 120;
    o[12] = s_tot[T_WITH];                                             // a 1-bar window is a bar with notes
    o[13] = s_tot[T_W4];
    o[14] = 0;
    o[15] = 0;
    status[b] = MHM_OK;
  }
}

}  // namespace

extern "C" int mhm_structure_counts(const int32_t* notes, const int32_t* counts3, const int32_t* meta, const int32_t* valid,
                                    const double* xlog2x, int32_t* out_counts, double* out_entropy, int32_t* bars, int32_t* status,
                                    int B, int max_notes, int max_bars, mh_stream_t stream) {
  MH_CHECK_ARG(notes && counts3 && meta && xlog2x && out_counts && out_entropy && status && B > 0,
               "structure_counts: bad arguments (a NULL pointer or B < 1)");
  MH_CHECK_ARG(max_notes >= 1 && max_notes <= MAX_NOTES, "structure_counts: max_notes in 1..%d (got %d)", MAX_NOTES, max_notes);
  MH_CHECK_ARG(max_bars >= 1 && max_bars <= MAX_BARS, "structure_counts: max_bars in 1..%d (got %d)", MAX_BARS, max_bars);
  MH_LAUNCH(structure_counts_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, notes, counts3, meta, valid, xlog2x, out_counts,
            out_entropy, bars, status, max_notes, max_bars);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
