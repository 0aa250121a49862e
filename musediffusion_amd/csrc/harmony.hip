// Chord-fit counts on the device (include/musehip_harmony.h): for every decoded row, how many notes are judged by a chord, how many of
// those are chord tones, how many notes lie in the key's scale, the same by sounding ticks, a pitch-class histogram and a per-bar table.
// Not in the reference: its metric.py stops at pitch and velocity.  The input is what decode_events_kernel (decode.hip) writes.
// Conventions of decode.hip and infill.hip: one 256-thread block per row, the chord list in LDS, int32 in and out, asynchronous on the
// given stream, no allocation.  Latency-bound integer work - no MFMA shape here.
//
// The chord at a note's onset judges the whole note: a note that sounds across a chord change is not split.
//
// Memory safety: n <= max_notes and c <= max_chords <= MAX_CHORDS are part of the status, decided before a list is touched; every LDS
// index is below c, 4 max_bars or 12 by construction and every global index is inside its row.
#include "common.h"
#include "../../include/musehip_harmony.h"

namespace {

constexpr int TB = 256;
constexpr int MAX_NOTES = 32768, MAX_CHORDS = 4096, MAX_BARS = 512;
constexpr int NSUM = 7;   // notes, judged, chord tones, scale tones, ticks of all / judged / chord-tone notes

// interval sets as 12-bit masks over the root: bit i = the pitch class i semitones above it
constexpr unsigned bits(int a, int b, int c, int d = -1) { return (1u << a) | (1u << b) | (1u << c) | (d >= 0 ? 1u << d : 0u); }
__device__ __forceinline__ unsigned quality_mask(int q) {
  switch (q) {
    case 0: return bits(0, 4, 7);        // ""
    case 1: return bits(0, 4, 7, 10);    // 7
    case 2: return bits(0, 4, 8);        // +
    case 3: return bits(0, 3, 6);        // dim
    case 4: return bits(0, 3, 7);        // m
    case 5: return bits(0, 3, 7, 10);    // m7
    case 6: return bits(0, 3, 6, 10);    // m7b5
    case 7: return bits(0, 4, 7, 11);    // maj7
    default: return bits(0, 5, 7);       // sus4
  }
}
constexpr unsigned MAJOR = bits(0, 2, 4, 5) | bits(7, 9, 11), MINOR = bits(0, 2, 3, 5) | bits(7, 8, 10);

// block-wide sums of NSUM values and the maximum of one, returned to every thread
__device__ __forceinline__ void block_reduce(int (&s)[NSUM], int& mx, int (*red)[4]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] += __shfl_xor(s[k], o, 64);
    const int u = __shfl_xor(mx, o, 64);
    mx = u > mx ? u : mx;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) red[k][wave] = s[k];
    red[NSUM][wave] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NSUM; ++k) s[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
  mx = red[NSUM][0];
#pragma unroll
  for (int w = 1; w < 4; ++w) mx = red[NSUM][w] > mx ? red[NSUM][w] : mx;
}

__global__ __launch_bounds__(TB) void harmony_counts_kernel(const int32_t* __restrict__ notes, const int32_t* __restrict__ chords,
                                                           const int32_t* __restrict__ counts3, const int32_t* __restrict__ meta,
                                                           const int32_t* __restrict__ valid, int32_t* __restrict__ out_counts,
                                                           int32_t* __restrict__ hist, int32_t* __restrict__ bars,
                                                           int32_t* __restrict__ status, int max_notes, int max_chords, int max_bars) {
  __shared__ int32_t ctick[MAX_CHORDS];
  __shared__ int32_t ctok[MAX_CHORDS];
  __shared__ int sbars[MAX_BARS * 4];
  __shared__ int red[NSUM + 1][4];
  __shared__ int hred[12][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int32_t* obars = bars ? bars + (int64_t)b * max_bars * 4 : nullptr;

  // ---- the status: one word per block, decided before anything is written and before a list is read
  int st = MHH_OK, n = 0, c = 0, tpb = 1, tonic = 0;
  unsigned scale = 0;
  if (valid && valid[b] == 0) {
    st = MHH_MASKED;
  } else {
    const int32_t key = meta[b * 11 + 1], ts = meta[b * 11 + 2];
    if (!(key >= 602 && key <= 625 && ts >= 627 && ts <= 630)) {
      st = MHH_BAD_META;
    } else {
      n = counts3[b * 3 + 0];
      c = counts3[b * 3 + 1];
      if (n < 0 || n > max_notes || c < 0 || c > max_chords) st = MHH_BAD_COUNTS;
      tpb = 480 * (ts == 627 ? 4 : (ts == 630 ? 6 : 3));            // decode_events_kernel's beats per bar
      tonic = (key - 602) % 12;
      scale = key >= 614 ? MINOR : MAJOR;
    }
  }
  if (st != MHH_OK) {                                                // uniform
    if (tid < 8) out_counts[b * 8 + tid] = 0;
    if (hist && tid < 12) hist[b * 12 + tid] = 0;
    if (obars)
      for (int i = tid; i < max_bars * 4; i += TB) obars[i] = 0;
    if (tid == 0) status[b] = st;
    return;
  }

  // ---- the chord list into LDS; is it sorted by tick?
  const int32_t* crow = chords + (int64_t)b * max_chords * 2;
  for (int j = tid; j < c; j += TB) {
    int32_t e[2];
    __builtin_memcpy(e, crow + 2 * j, 8);
    ctick[j] = e[0];
    ctok[j] = e[1];
  }
  if (obars)
    for (int i = tid; i < max_bars * 4; i += TB) sbars[i] = 0;
  __syncthreads();
  int falls = 0;
  for (int j = tid + 1; j < c; j += TB) falls |= ctick[j] < ctick[j - 1];
  const bool sorted = !__syncthreads_or(falls);

  // ---- one note per thread and pass
  int s[NSUM] = {0, 0, 0, 0, 0, 0, 0}, top = -1, h[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t* nrow = notes + (int64_t)b * max_notes * 4;
  for (int j0 = 0; j0 < n; j0 += TB) {                               // uniform trip count: the ballots below need every lane
    const int j = j0 + tid;
    const bool live = j < n;
    int pc = -1;
    if (live) {
      int32_t v[4];
      // one load of the whole note; a row of a packed batch is only 4-byte aligned, and the velocity is not used, so the compiler
      // makes it one global_load_dwordx3
      __builtin_memcpy(v, nrow + 4 * (int64_t)j, 16);
      const int32_t start = v[0], end = v[1];
      pc = v[2] % 12;
      pc = pc < 0 ? pc + 12 : pc;
      int at = -1;                                                   // the chord in force
      if (sorted) {                                                  // the last entry with tick <= start
        int lo = 0, hi = c;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (ctick[mid] <= start) lo = mid + 1; else hi = mid;
        }
        at = lo - 1;
      } else {                                                       // the largest tick <= start, the last of equals
        int32_t best = 0;
        for (int k = 0; k < c; ++k) {
          const int32_t t = ctick[k];
          if (t <= start && (at < 0 || t >= best)) { at = k; best = t; }
        }
      }
      int judged = 0, tone = 0;
      if (at >= 0) {
        const int32_t tok = ctok[at];
        if (tok >= 195 && tok <= 302) {
          const int r = (tok - 195) / 9, q = (tok - 195) % 9;
          int rel = pc - (9 + r) % 12;
          rel = rel < 0 ? rel + 12 : rel;
          judged = 1;
          tone = (quality_mask(q) >> rel) & 1;
        }
      }
      int rel = pc - tonic;
      rel = rel < 0 ? rel + 12 : rel;
      const int in_scale = (scale >> rel) & 1;
      long long len = (long long)end - start;
      len = len < 0 ? 0 : (len > 65535 ? 65535 : len);
      s[0] += 1; s[1] += judged; s[2] += tone; s[3] += in_scale;
      s[4] += (int)len; s[5] += judged ? (int)len : 0; s[6] += tone ? (int)len : 0;
      if (start >= 0) {
        const int k = start / tpb;
        top = k > top ? k : top;
        if (obars && k < max_bars) {                                 // integer sums: the order of the LDS atomics does not matter
          atomicAdd(&sbars[k * 4 + 0], 1);
          if (judged) atomicAdd(&sbars[k * 4 + 1], 1);
          if (tone) atomicAdd(&sbars[k * 4 + 2], 1);
          if (in_scale) atomicAdd(&sbars[k * 4 + 3], 1);
        }
      }
    }
    if (hist) {                                                      // uniform
#pragma unroll
      for (int p = 0; p < 12; ++p) h[p] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(pc == p));   // the wave's count, in every lane
    }
  }
  block_reduce(s, top, red);                                         // its barrier also closes the LDS atomics
  if (hist) {
    if ((tid & 63) == 0) {
#pragma unroll
      for (int p = 0; p < 12; ++p) hred[p][tid >> 6] = h[p];
    }
    __syncthreads();
    if (tid < 12) hist[b * 12 + tid] = hred[tid][0] + hred[tid][1] + hred[tid][2] + hred[tid][3];
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) out_counts[b * 8 + k] = s[k];
    out_counts[b * 8 + 7] = top + 1;
    status[b] = MHH_OK;
  }
  if (obars)
    for (int i = tid; i < max_bars * 4; i += TB) obars[i] = sbars[i];
}

}  // namespace

extern "C" int mhh_harmony_counts(const int32_t* notes, const int32_t* chords, const int32_t* counts3, const int32_t* meta,
                                  const int32_t* valid, int32_t* out_counts, int32_t* hist, int32_t* bars, int32_t* status, int B,
                                  int max_notes, int max_chords, int max_bars, mh_stream_t stream) {
  MH_CHECK_ARG(notes && chords && counts3 && meta && out_counts && status && B > 0,
               "harmony_counts: bad arguments (a NULL pointer or B < 1)");
  MH_CHECK_ARG(max_notes >= 1 && max_notes <= MAX_NOTES, "harmony_counts: max_notes in 1..%d (got %d)", MAX_NOTES, max_notes);
  MH_CHECK_ARG(max_chords >= 1 && max_chords <= MAX_CHORDS, "harmony_counts: max_chords in 1..%d (got %d)", MAX_CHORDS, max_chords);
  MH_CHECK_ARG(max_bars >= 0 && max_bars <= MAX_BARS, "harmony_counts: max_bars in 0..%d (got %d)", MAX_BARS, max_bars);
  MH_CHECK_ARG((bars != nullptr) == (max_bars > 0), "harmony_counts: a bars table needs max_bars > 0 and max_bars > 0 a table (got %s, max_bars = %d)",
               bars ? "a table" : "NULL", max_bars);
  MH_LAUNCH(harmony_counts_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, notes, chords, counts3, meta, valid, out_counts, hist, bars,
            status, max_notes, max_chords, max_bars);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
