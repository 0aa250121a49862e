// Interplay counts on the device (include/musehip_arrange.h): the rows of a batch grouped into songs, and for every row the notes
// that sound together with a note of another row of its song - per interval class and per "this row is below / above" the number of
// such pairs and their common ticks.  Not in the reference: it never looks at two rows together in time.  The input is what
// decode_events_kernel (decode.hip) writes.  Conventions of harmony.hip and structure.hip: one 256-thread block per row, int32 in,
// asynchronous on the given stream, no allocation.  The join itself has the form of pairstats.hip: the partner's list goes through
// LDS in tiles, the tile after the one in work is on its way in registers, every thread holds its own query in registers and reads
// the tile's notes as broadcasts.  Integer compare-and-add work - no MFMA shape here.
//
// A note is brought into one form on the way into LDS and into the query register: (start + shift, end + shift, pitch, 1) when it
// is counted, EMPTY = (INT_MAX, 0, 0, 0) when it is not, so that the inner loop is one overlap test: an empty note overlaps nothing
// (min(end) >= 0, max(start) = INT_MAX).  That rewrite is why the tiles are staged through registers and not by the LDS-DMA of
// lds_dma.h, which moves bytes as they are: it would need a second pass over every tile and a second barrier.
//
// Bit-for-bit by construction: every sum is an integer.  Within a tile a thread adds into int32 (at most KT pairs of at most 65535
// ticks: below 2^25), after the tile into int64; the block folds with shuffles and one LDS round.
//
// Memory safety: n <= max_notes is part of a row's status and of "in range", decided before a list is touched; a list is read at
// j < n only; B * max_notes <= 2^31 notes are indexed in 64 bits; LDS indices are tid, tid + TB < KT and j < min(KT, n - j0).
#include "common.h"
#include "../../include/musehip_arrange.h"

namespace {

constexpr int TB = 256;
constexpr int NW = TB / 64;         // waves per block
constexpr int KT = 512;             // partner notes per tile == mha_key_tile()
constexpr int PRE = KT / TB;        // notes of a tile each thread moves
constexpr int MAX_NOTES = 32768;
constexpr int MAX_TICK = 1 << 29;   // the largest end tick and the largest shift: a shifted time stays below 2^31
constexpr int CLAMP = 65535;        // ticks one pair adds at most
constexpr int NRED = 20;            // 9 pair sums, 9 tick sums, counted, accompanied
static_assert(KT % TB == 0 && (int64_t)KT * CLAMP < (1ll << 31), "a tile's sums fit int32");

__device__ __forceinline__ int4 empty_note() { return make_int4(0x7fffffff, 0, 0, 0); }

// the note at p in the form of the join (the header's step 4): shifted when counted, EMPTY when skipped
__device__ __forceinline__ int4 load_note(const int32_t* __restrict__ p, int shift) {
  int32_t v[4];
  __builtin_memcpy(v, p, 16);                                           // the whole note in one load (harmony.hip)
  const bool counted = v[2] >= 0 && v[2] <= 127 && v[0] >= 0 && v[0] < v[1] && v[1] <= MAX_TICK;
  return counted ? make_int4(v[0] + shift, v[1] + shift, v[2], 1) : empty_note();
}

__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Rows {
  const int32_t* __restrict__ counts3;
  const int32_t* __restrict__ valid;
  const int32_t* __restrict__ song;
  const int32_t* __restrict__ shift;
  int max_notes;
  __device__ __forceinline__ int notes_of(int64_t c) const { return counts3[c * 3]; }
  __device__ __forceinline__ int shift_of(int64_t c) const { return shift ? shift[c] : 0; }
  __device__ __forceinline__ int song_of(int64_t c) const { return song ? song[c] : 0; }
  // the header's step 1
  __device__ __forceinline__ bool in_range(int64_t c) const {
    if (valid && valid[c] == 0) return false;
    const int n = notes_of(c), s = shift_of(c);
    return n >= 0 && n <= max_notes && s >= 0 && s <= MAX_TICK;
  }
};

__global__ __launch_bounds__(TB) void interplay_counts_kernel(const int32_t* __restrict__ notes, const int32_t* __restrict__ counts3,
                                                             const int32_t* __restrict__ meta, const int32_t* __restrict__ valid,
                                                             const int32_t* __restrict__ song, const int32_t* __restrict__ shift,
                                                             int32_t* __restrict__ out_counts, long long* __restrict__ out_pairs,
                                                             long long* __restrict__ out_ticks, int32_t* __restrict__ status, int B,
                                                             int max_notes) {
  __shared__ int4 tile[2][KT];
  __shared__ int row_notes[TB];                                        // of the TB rows in work: n_c of a partner, -1 otherwise
  __shared__ int row_shift[TB];
  __shared__ long long red[NW][NRED];
  __shared__ int s_partners[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const Rows rows{counts3, valid, song, shift, max_notes};

  // ---- the status: one word per block.  MASKED, BAD_COUNTS, BAD_SHIFT need the row alone
  int st = MHA_OK, n = 0, sb = 0;
  if (valid && valid[b] == 0) {
    st = MHA_MASKED;
  } else {
    n = rows.notes_of(b);
    sb = rows.shift_of(b);
    if (n < 0 || n > max_notes) st = MHA_BAD_COUNTS;
    else if (sb < 0 || sb > MAX_TICK) st = MHA_BAD_SHIFT;
  }
  // ---- the partners and MIXED: the block looks at every row of the batch once
  const int gb = rows.song_of(b);
  int partners = 0;
  if (st == MHA_OK) {                                                   // uniform
    const int32_t m0 = meta[b * 11 + 0], m1 = meta[b * 11 + 1], m2 = meta[b * 11 + 2];
    int mine = 0, mixed = 0;
    for (int64_t c = tid; c < B; c += TB) {
      if (c == b || rows.song_of(c) != gb || !rows.in_range(c)) continue;
      ++mine;
      mixed |= meta[c * 11 + 0] != m0 || meta[c * 11 + 1] != m1 || meta[c * 11 + 2] != m2;
    }
    mine = (int)wave_sum64(mine);
    if (lane == 0) s_partners[wave] = mine;
    if (__syncthreads_or(mixed)) st = MHA_MIXED;
    partners = s_partners[0] + s_partners[1] + s_partners[2] + s_partners[3];
  }
  if (st != MHA_OK) {                                                   // uniform
    if (tid < 8) out_counts[b * 8 + tid] = 0;
    if (tid < 9) out_pairs[b * 9 + tid] = 0;
    if (tid < 9) out_ticks[b * 9 + tid] = 0;
    if (tid == 0) status[b] = st;
    return;
  }

  long long pairs[9], ticks[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) pairs[c] = ticks[c] = 0;
  int counted = 0, accompanied = 0;
  unsigned turn = 0;                                                    // tiles staged so far: the LDS buffer alternates
  const int32_t* __restrict__ nrow = notes + b * max_notes * 4;

  // ---- one note per thread and pass
  for (int q0 = 0; q0 < n; q0 += TB) {
    const int4 x = q0 + tid < n ? load_note(nrow + 4 * (int64_t)(q0 + tid), sb) : empty_note();
    counted += x.w;
    int met = 0;
    for (int64_t c0 = 0; partners > 0 && c0 < B; c0 += TB) {
      __syncthreads();                                                  // the last TB rows are done with
      {
        const int64_t c = c0 + tid;
        const bool partner = c < B && c != b && rows.song_of(c) == gb && rows.in_range(c);
        row_notes[tid] = partner ? rows.notes_of(c) : -1;
        row_shift[tid] = partner ? rows.shift_of(c) : 0;
      }
      __syncthreads();
      const int here = (int)(B - c0 < TB ? B - c0 : TB);
      for (int i = 0; i < here; ++i) {
        const int pn = row_notes[i];                                    // uniform
        if (pn <= 0) continue;
        const int ps = row_shift[i];
        const int32_t* __restrict__ prow = notes + (c0 + i) * max_notes * 4;
        // a tile is one contiguous run of the partner's list: thread t moves its notes t, t + TB, ...
        int4 pre[PRE];
        auto fetch = [&](int j0) {
#pragma unroll
          for (int k = 0; k < PRE; ++k) {
            const int j = j0 + tid + k * TB;
            pre[k] = j < pn ? load_note(prow + 4 * (int64_t)j, ps) : empty_note();
          }
        };
        fetch(0);
        for (int j0 = 0; j0 < pn; j0 += KT) {
          int4* __restrict__ t = tile[turn++ & 1];
#pragma unroll
          for (int k = 0; k < PRE; ++k) t[tid + k * TB] = pre[k];
          __syncthreads();                                              // the other buffer stays free until the next barrier
          if (j0 + KT < pn) fetch(j0 + KT);                             // in flight while this tile is worked on
          const int cnt = pn - j0 < KT ? pn - j0 : KT;
          int tp[9], tt[9];
#pragma unroll
          for (int c = 0; c < 9; ++c) tp[c] = tt[c] = 0;
#pragma unroll 4
          for (int j = 0; j < cnt; ++j) {
            const int4 y = t[j];                                        // one address for the whole block: a broadcast
            const int o = min(x.y, y.y) - max(x.x, y.x);                // an empty note on either side: o <= -INT_MAX + end < 0
            if (o <= 0) continue;
            const int common = min(o, CLAMP);
            const int dp = x.z - y.z;
            const unsigned d = (unsigned)(dp < 0 ? -dp : dp) % 12u;
            const int ic = (int)(d > 6u ? 12u - d : d);
            met = 1;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
              tp[c] += ic == c;
              tt[c] += ic == c ? common : 0;
            }
            tp[7] += dp < 0;
            tt[7] += dp < 0 ? common : 0;
            tp[8] += dp > 0;
            tt[8] += dp > 0 ? common : 0;
          }
#pragma unroll
          for (int c = 0; c < 9; ++c) {
            pairs[c] += tp[c];
            ticks[c] += tt[c];
          }
        }
      }
    }
    accompanied += met;
  }

  // ---- fold: shuffles within a wave, one LDS round across the waves, one thread per column stores
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const long long p = wave_sum64(pairs[c]), t = wave_sum64(ticks[c]);
    if (lane == 0) {
      red[wave][c] = p;
      red[wave][9 + c] = t;
    }
  }
  {
    const long long a = wave_sum64(counted), m = wave_sum64(accompanied);
    if (lane == 0) {
      red[wave][18] = a;
      red[wave][19] = m;
    }
  }
  __syncthreads();
  if (tid < NRED) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][tid];
    if (tid < 9) out_pairs[b * 9 + tid] = v;
    else if (tid < 18) out_ticks[b * 9 + tid - 9] = v;
    else if (tid == 18) {
      out_counts[b * 8 + 0] = (int)v;
      out_counts[b * 8 + 1] = n - (int)v;
    } else {
      out_counts[b * 8 + 2] = partners;
      out_counts[b * 8 + 3] = (int)v;
    }
  }
  if (tid >= 32 && tid < 36) out_counts[b * 8 + 4 + tid - 32] = 0;
  if (tid == 0) status[b] = MHA_OK;
}

}  // namespace

extern "C" int mha_key_tile(void) { return KT; }

extern "C" int mha_interplay_counts(const int32_t* notes, const int32_t* counts3, const int32_t* meta, const int32_t* valid,
                                    const int32_t* song, const int32_t* shift, int32_t* out_counts, int64_t* out_pairs,
                                    int64_t* out_ticks, int32_t* status, int B, int max_notes, mh_stream_t stream) {
  MH_CHECK_ARG(notes && counts3 && meta && out_counts && out_pairs && out_ticks && status && B > 0,
               "interplay_counts: bad arguments (a NULL pointer or B < 1)");
  MH_CHECK_ARG(max_notes >= 1 && max_notes <= MAX_NOTES, "interplay_counts: max_notes in 1..%d (got %d)", MAX_NOTES, max_notes);
  MH_CHECK_ARG((int64_t)B * max_notes <= (1ll << 31), "interplay_counts: B * max_notes = %lld exceeds 2^31",
               (long long)B * max_notes);
  MH_LAUNCH(interplay_counts_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, notes, counts3, meta, valid, song, shift, out_counts,
            (long long*)out_pairs, (long long*)out_ticks, status, B, max_notes);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
