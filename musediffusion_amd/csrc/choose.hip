// Choosing each song's tracks among sampled candidates (include/musehip_choose.h): a candidate batch holds S songs x T tracks x K
// candidates.  pair_fit_kernel is the all-pairs join of arrange.hip with the sums kept apart per pair of rows: for every row the notes
// that sound together with a note of every row of ANOTHER track of its song, per interval class the number of such pairs and their
// common ticks.  choose_kernel is the search: per song the admissible combinations of one candidate a track, each scored from a table
// of pair scores in LDS, the best one kept.  Not in the reference: it samples every track once.  Conventions of arrange.hip: int32
// in, asynchronous on the given stream, no allocation, integer compare-and-add work - no MFMA shape here.
//
// pair_fit_kernel: one 256-thread block per row.  A note is brought into one form on the way into LDS and into the query register:
// (start + shift, end + shift, pitch, 1) when it is counted, EMPTY = (INT_MAX, 0, 0, 0) when it is not, so that the inner loop is one
// overlap test (arrange.hip).  The block walks the R rows of its song in the order of their local index; a partner's list goes through
// LDS in tiles, the tile after the one in work on its way in registers, every thread reads the tile's notes as broadcasts; behind a
// partner's last tile the block folds and one thread per column stores.  A row that is no partner costs fourteen stores of zero.
//
// Bit-for-bit by construction: every sum is an integer.  Within a tile a thread adds into int32 (at most KT pairs of at most 65535
// ticks: below 2^25), after the tile into int64.
//
// Memory safety: n <= max_notes is part of a row's status and of "in range", decided before a list is touched; a list is read at
// j < n only; B * max_notes <= 2^31 notes and B * R * 7 outputs are indexed in 64 bits; LDS indices are r < R <= MAX_R, tid,
// tid + TB < KT and j < min(KT, n - j0).  choose_kernel: R <= CH_MAX_R is what K^T <= 2^20 leaves (checked on the host, with the
// table's size); LDS indices are r < R, t < T and m < the number of combinations.
#include "common.h"
#include "../../include/musehip_choose.h"

namespace {

constexpr int TB = 256;
constexpr int NW = TB / 64;         // waves per block
constexpr int KT = 512;             // partner notes per tile == mhac_key_tile()
constexpr int PRE = KT / TB;        // notes of a tile each thread moves
constexpr int MAX_NOTES = 32768;
constexpr int MAX_TICK = 1 << 29;   // the largest end tick and the largest shift: a shifted time stays below 2^31
constexpr int CLAMP = 65535;        // ticks one pair adds at most
constexpr int NCLS = 7;             // interval classes
constexpr int MAX_T = MHAC_MAX_TRACKS, MAX_K = MHAC_MAX_CANDIDATES;
constexpr int MAX_R = MAX_T * MAX_K;
static_assert(KT % TB == 0 && (int64_t)KT * CLAMP < (1ll << 31), "a tile's sums fit int32");

__device__ __forceinline__ int4 empty_note() { return make_int4(0x7fffffff, 0, 0, 0); }

// the note at p in the form of the join (the header's step 4): shifted when counted, EMPTY when skipped
__device__ __forceinline__ int4 load_note(const int32_t* __restrict__ p, int shift) {
  int32_t v[4];
  __builtin_memcpy(v, p, 16);
  const bool counted = v[2] >= 0 && v[2] <= 127 && v[0] >= 0 && v[0] < v[1] && v[1] <= MAX_TICK;
  return counted ? make_int4(v[0] + shift, v[1] + shift, v[2], 1) : empty_note();
}

__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(TB) void pair_fit_kernel(const int32_t* __restrict__ notes, const int32_t* __restrict__ counts3,
                                                     const int32_t* __restrict__ meta, const int32_t* __restrict__ valid,
                                                     const int32_t* __restrict__ shift, long long* __restrict__ out_ticks,
                                                     long long* __restrict__ out_pairs, int32_t* __restrict__ status, int T, int K,
                                                     int max_notes) {
  __shared__ int4 tile[2][KT];
  __shared__ int row_notes[MAX_R];                                     // of the song's rows: n_c of a partner, -1 otherwise
  __shared__ int row_shift[MAX_R];
  __shared__ long long red[NW][2 * NCLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = T * K;
  const int64_t b = blockIdx.x;
  const int64_t base = b / R * R;                                       // the song's first row
  const int lb = (int)(b - base), tb = lb / K;

  // ---- the status: one word per block.  MASKED, BAD_COUNTS, BAD_SHIFT need the row alone
  int st = MHA_OK, n = 0, sb = 0;
  if (valid && valid[b] == 0) {
    st = MHA_MASKED;
  } else {
    n = counts3[b * 3];
    sb = shift ? shift[b] : 0;
    if (n < 0 || n > max_notes) st = MHA_BAD_COUNTS;
    else if (sb < 0 || sb > MAX_TICK) st = MHA_BAD_SHIFT;
  }
  // ---- the partners and MIXED: the block looks at every row of its song once
  if (st == MHA_OK) {                                                   // uniform
    const int32_t m0 = meta[b * 11 + 0], m1 = meta[b * 11 + 1], m2 = meta[b * 11 + 2];
    int mixed = 0;
    for (int r = tid; r < R; r += TB) {
      const int64_t c = base + r;
      int pn = -1, ps = 0;
      if (r / K != tb && !(valid && valid[c] == 0)) {
        const int cn = counts3[c * 3], cs = shift ? shift[c] : 0;
        if (cn >= 0 && cn <= max_notes && cs >= 0 && cs <= MAX_TICK) {
          pn = cn;
          ps = cs;
          mixed |= meta[c * 11 + 0] != m0 || meta[c * 11 + 1] != m1 || meta[c * 11 + 2] != m2;
        }
      }
      row_notes[r] = pn;
      row_shift[r] = ps;
    }
    if (__syncthreads_or(mixed)) st = MHA_MIXED;                        // and row_notes / row_shift are in place
  }
  long long* __restrict__ oticks = out_ticks + b * R * NCLS;
  long long* __restrict__ opairs = out_pairs + b * R * NCLS;
  if (st != MHA_OK) {                                                   // uniform
    for (int i = tid; i < R * NCLS; i += TB) oticks[i] = opairs[i] = 0;
    if (tid == 0) status[b] = st;
    return;
  }

  const int32_t* __restrict__ nrow = notes + b * max_notes * 4;
  const int4 x0 = tid < n ? load_note(nrow + 4 * (int64_t)tid, sb) : empty_note();   // the first pass's note stays in registers
  unsigned turn = 0;                                                    // tiles staged so far: the LDS buffer alternates

  for (int r = 0; r < R; ++r) {
    const int pn = row_notes[r];                                        // uniform
    if (pn <= 0 || n == 0) {                                            // no partner, or nothing to meet: zeros
      if (tid < NCLS) oticks[r * NCLS + tid] = 0;
      else if (tid < 2 * NCLS) opairs[r * NCLS + tid - NCLS] = 0;
      continue;
    }
    const int ps = row_shift[r];
    const int32_t* __restrict__ prow = notes + (base + r) * max_notes * 4;
    long long pairs[NCLS], ticks[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) pairs[c] = ticks[c] = 0;
    // ---- one note per thread and pass
    for (int q0 = 0; q0 < n; q0 += TB) {
      const int4 x = q0 == 0 ? x0 : (q0 + tid < n ? load_note(nrow + 4 * (int64_t)(q0 + tid), sb) : empty_note());
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
        __syncthreads();                                                // the other buffer stays free until the next barrier
        if (j0 + KT < pn) fetch(j0 + KT);                               // in flight while this tile is worked on
        const int cnt = pn - j0 < KT ? pn - j0 : KT;
        int tp[NCLS], tt[NCLS];
#pragma unroll
        for (int c = 0; c < NCLS; ++c) tp[c] = tt[c] = 0;
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
          const int4 y = t[j];                                          // one address for the whole block: a broadcast
          const int o = min(x.y, y.y) - max(x.x, y.x);                  // an empty note on either side: o < 0
          if (o <= 0) continue;
          const int common = min(o, CLAMP);
          const int dp = x.z - y.z;
          const unsigned d = (unsigned)(dp < 0 ? -dp : dp) % 12u;
          const int ic = (int)(d > 6u ? 12u - d : d);
#pragma unroll
          for (int c = 0; c < NCLS; ++c) {
            tp[c] += ic == c;
            tt[c] += ic == c ? common : 0;
          }
        }
#pragma unroll
        for (int c = 0; c < NCLS; ++c) {
          pairs[c] += tp[c];
          ticks[c] += tt[c];
        }
      }
    }
    // ---- the fold of this partner: shuffles within a wave, one LDS round across the waves, one thread per column stores.  red is
    // free: its readers of the partner before passed at least one barrier of the tile loop since (pn > 0 and n > 0: a tile at least)
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      const long long t = wave_sum64(ticks[c]), p = wave_sum64(pairs[c]);
      if (lane == 0) {
        red[wave][c] = t;
        red[wave][NCLS + c] = p;
      }
    }
    __syncthreads();
    if (tid < 2 * NCLS) {
      long long v = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += red[w][tid];
      if (tid < NCLS) oticks[r * NCLS + tid] = v;
      else opairs[r * NCLS + tid - NCLS] = v;
    }
  }
  if (tid == 0) status[b] = MHA_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the search
constexpr int CH_MAX_R = 80;                                            // the largest T * K with K^T <= 2^20 and K <= 16: T = 5, K = 16
constexpr long long SCORE_MAX = 1ll << 40;

__global__ __launch_bounds__(TB) void choose_kernel(const long long* __restrict__ W, const long long* __restrict__ unary,
                                                   const int32_t* __restrict__ eligible, int32_t* __restrict__ choice,
                                                   long long* __restrict__ best, long long* __restrict__ first,
                                                   int32_t* __restrict__ status, int T, int K) {
  __shared__ long long w[CH_MAX_R * CH_MAX_R];                          // the song's table
  __shared__ long long un[CH_MAX_R];
  __shared__ unsigned char el[CH_MAX_R];
  __shared__ unsigned char list[MAX_T][MAX_K];                          // per kept track, in the order of the tracks: its eligible k, ascending
  __shared__ int radix[MAX_T], track_of[MAX_T];                         // ... how many, and which track it is
  __shared__ int s_kept, s_total;
  __shared__ long long red_v[NW];
  __shared__ int red_m[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = T * K;
  const int64_t s = blockIdx.x;

  for (int r = tid; r < R; r += TB) {
    el[r] = eligible ? eligible[s * R + r] != 0 : 1;
    un[r] = unary ? unary[s * R + r] : 0;
  }
  const long long* __restrict__ Ws = W + s * R * R;
  for (int i = tid; i < R * R; i += TB) w[i] = Ws[i];
  __syncthreads();
  // ---- an entry that would be read outside +-2^40?  unary of an eligible row, W of two eligible rows, the lower track first
  int bad = 0;
  for (int r = tid; r < R; r += TB) bad |= el[r] && (un[r] > SCORE_MAX || un[r] < -SCORE_MAX);
  for (int i = tid; i < R * R; i += TB) {
    const int r = i / R, c = i - r * R;
    bad |= r / K < c / K && el[r] && el[c] && (w[i] > SCORE_MAX || w[i] < -SCORE_MAX);
  }
  // ---- the kept tracks and their lists: one thread, at most 320 steps
  if (tid == 0) {
    int kept = 0, total = 1;
    for (int t = 0; t < T; ++t) {
      int e = 0;
      for (int k = 0; k < K; ++k)
        if (el[t * K + k]) list[kept][e++] = (unsigned char)k;
      if (e) {
        radix[kept] = e;
        track_of[kept++] = t;
        total *= e;                                                     // <= K^T <= 2^20
      }
    }
    s_kept = kept;
    s_total = total;
  }
  bad = __syncthreads_or(bad);
  const int kept = s_kept, total = s_total;
  if (bad || kept == 0) {                                               // uniform
    for (int t = tid; t < T; t += TB) choice[s * T + t] = -1;
    if (tid == 0) {
      best[s] = 0;
      first[s] = 0;
      status[s] = bad ? MHAC_BAD_SCORE : MHAC_EMPTY;
    }
    return;
  }

  // ---- the combinations in the order of q: m counts them with the kept tracks' lists as digits, the lowest track first, which is q's
  // order since a list ascends.  A thread takes m = tid, tid + TB, ...: its own m ascend, so `>` keeps the smallest on a tie
  long long bv = 0;
  int bm = -1;
  for (int m = tid; m < total; m += TB) {
    int rows[MAX_T];
    int rest = m;
    long long v = 0;
#pragma unroll
    for (int i = 0; i < MAX_T; ++i) {
      if (i < kept) {                                                   // uniform
        const int e = radix[i];
        const int d = rest % e;
        rest /= e;
        const int r = track_of[i] * K + list[i][d];
        rows[i] = r;
        v += un[r];
#pragma unroll
        for (int j = 0; j < i; ++j) v += w[rows[j] * R + r];
      }
    }
    if (bm < 0 || v > bv) {
      bv = v;
      bm = m;
    }
    if (m == 0) first[s] = v;                                           // thread 0's first combination: the smallest admissible q
  }
  // ---- fold (objective, m): the larger objective, on a tie the smaller m; a thread without a combination has m = -1
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ov = __shfl_xor(bv, o, 64);
    const int om = __shfl_xor(bm, o, 64);
    if (om >= 0 && (bm < 0 || ov > bv || (ov == bv && om < bm))) {
      bv = ov;
      bm = om;
    }
  }
  if (lane == 0) {
    red_v[wave] = bv;
    red_m[wave] = bm;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < NW; ++k) {
      const long long ov = red_v[k];
      const int om = red_m[k];
      if (om >= 0 && (bm < 0 || ov > bv || (ov == bv && om < bm))) {
        bv = ov;
        bm = om;
      }
    }
    best[s] = bv;
    status[s] = kept == T ? MHAC_OK : MHAC_PARTIAL;
    for (int t = 0; t < T; ++t) choice[s * T + t] = -1;
    int rest = bm;
    for (int i = 0; i < kept; ++i) {
      const int e = radix[i];
      choice[s * T + track_of[i]] = list[i][rest % e];
      rest /= e;
    }
  }
}

}  // namespace

extern "C" int mhac_key_tile(void) { return KT; }

extern "C" int mhac_pair_fit(const int32_t* notes, const int32_t* counts3, const int32_t* meta, const int32_t* valid,
                             const int32_t* shift, int64_t* out_ticks, int64_t* out_pairs, int32_t* status, int S, int T, int K,
                             int max_notes, mh_stream_t stream) {
  MH_CHECK_ARG(notes && counts3 && meta && out_ticks && out_pairs && status && S > 0,
               "pair_fit: bad arguments (a NULL pointer or S < 1)");
  MH_CHECK_ARG(T >= 1 && T <= MAX_T && K >= 1 && K <= MAX_K, "pair_fit: T in 1..%d and K in 1..%d (got %d, %d)", MAX_T, MAX_K, T, K);
  MH_CHECK_ARG(max_notes >= 1 && max_notes <= MAX_NOTES, "pair_fit: max_notes in 1..%d (got %d)", MAX_NOTES, max_notes);
  const int64_t B = (int64_t)S * T * K;
  MH_CHECK_ARG(B * max_notes <= (1ll << 31) && B < (1ll << 31), "pair_fit: B * max_notes = %lld exceeds 2^31 (B = S * T * K = %lld)",
               (long long)B * max_notes, (long long)B);
  MH_LAUNCH(pair_fit_kernel, dim3((unsigned)B), dim3(TB), 0, (hipStream_t)stream, notes, counts3, meta, valid, shift,
            (long long*)out_ticks, (long long*)out_pairs, status, T, K, max_notes);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mhac_choose(const int64_t* W, const int64_t* unary, const int32_t* eligible, int32_t* choice, int64_t* best,
                           int64_t* first, int32_t* status, int S, int T, int K, mh_stream_t stream) {
  MH_CHECK_ARG(W && choice && best && first && status && S > 0, "choose: bad arguments (a NULL pointer or S < 1)");
  MH_CHECK_ARG(T >= 1 && T <= MAX_T && K >= 1 && K <= MAX_K, "choose: T in 1..%d and K in 1..%d (got %d, %d)", MAX_T, MAX_K, T, K);
  long long combos = 1;
  for (int t = 0; t < T && combos <= MHAC_MAX_COMBINATIONS; ++t) combos *= K;
  if (combos > MHAC_MAX_COMBINATIONS || T * K > CH_MAX_R) {
    mh_set_error("choose: K^T = %d^%d exceeds %d combinations: the search is exact enumeration (approximate search is not built)", K, T,
                 (int)MHAC_MAX_COMBINATIONS);
    return MH_ERR_UNSUPPORTED;
  }
  MH_LAUNCH(choose_kernel, dim3(S), dim3(TB), 0, (hipStream_t)stream, (const long long*)W, (const long long*)unary, eligible, choice,
            (long long*)best, (long long*)first, status, T, K);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
