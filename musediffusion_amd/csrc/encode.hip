// Notes + chord progression -> event words -> model rows, on the device: the inverse of decode.hip.
// Reference: commu/preprocessor/encoder/encoder.py:21-69 EventSequenceEncoder.encode and encoder_utils.py:184-368 (extract_events,
// read_items, group_items, item2event, insert_chord_on_event, detect_chord) from the note list onward; MuseDiffusion/data/preprocess.py:36-56
// merge_and_mask.  Conventions of decode.hip / batch.hip: one 256-thread block per row, the row's working set in LDS, scans by ballot or
// shuffle, int32 in and out, asynchronous on the given stream, no allocation.  Latency-bound integer work - no MFMA shape here.
//
// The reference sorts three times: the notes by (start, pitch), twice more (stably) by start, and at the end chord events + note events
// (stably) by time.  Here both are ONE bitonic network over (64-bit key, 32-bit index) pairs compared lexicographically.  A bitonic
// network alone is not stable; the index makes every pair distinct, so the network's result is the unique ascending order and equals the
// stable sort's: the notes by (start, pitch, input index), the events by (time, chord side before note side, place in its own list).
// The four events of a note (and the two of a chord change) share one time and are neighbours in their list, so they are sorted as one
// unit and expanded to words afterwards, by a block prefix scan over the units' word counts.
//
// Who decides: the status of a row is a function of values every thread of the block holds alike (the parameter block, the counts,
// block-reduced totals), so barriers inside `if (st == OK)` are uniform.
//
// Memory safety: n_notes / n_slots are checked against the buffers' capacities AND the LDS capacities before anything is indexed with
// them, every LDS index is below the capacity by construction (commented where it is not obvious), every global write is guarded by ld /
// cap, and a row whose counts or time base make no sense gets a status, not a pointer.
#include <climits>

#include "common.h"

// the chord side's float64 arithmetic must round where Python's does: no fused multiply-add (hipcc contracts by default).  The
// __dmul_rn / __dadd_rn / __ddiv_rn / __dsub_rn intrinsics below are never contracted; the pragma covers what a later edit might add.
#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;
constexpr int MAX_ROW = 4096;      // == mh_batch_max_row() (batch.hip); the wrappers check it
constexpr int MAX_NOTES = 2048;    // mh_encode_max_notes()
constexpr int MAX_SLOTS = 1024;    // mh_encode_max_slots()
constexpr int MAX_UNITS = 4096;    // measures + chord slots + notes of one row (a power of two: the network's size)
constexpr int MAX_T = 1 << 24;     // ticks per bar the integer formulas are proven for
constexpr int NOTE_BASE = 1 << 24; // unit index of the first note: above every chord-side index (measures * (slots + 1) < 2^23)
constexpr unsigned long long KEY_NONE = ~0ull;

// exclusive prefix sum of one small int per thread over the block; total to every thread
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + incl - v;
}

__device__ __forceinline__ long long block_sum(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const long long r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

__device__ __forceinline__ long long block_max(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = red[w] > r ? red[w] : r;
  __syncthreads();
  return r;
}

// ascending sort of (key[i], pay[i]), i < P (a power of two <= MAX_UNITS), by key, then pay.  Callers make the pairs distinct.
__device__ void bitonic_sort(unsigned long long* key, int32_t* pay, int P) {
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += TB) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));       // bit j clear; i | j < P
        const int l = i | j;
        const unsigned long long a = key[i], c = key[l];
        const int32_t pa = pay[i], pc = pay[l];
        const bool gt = a > c || (a == c && pa > pc);
        if (gt == ((i & k) == 0)) { key[i] = c; key[l] = a; pay[i] = pc; pay[l] = pa; }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int next_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// item2event of one note that starts in the bar at bar_st: (Position, Note Velocity, Note On, Note Duration), -1 = no word; the
// number of "OOV" lines the reference prints for it
__device__ __forceinline__ int note_words(int start, int end, int pitch, int vel, long long bar_st, int T, int32_t (&w)[4]) {
  int oov = 0;
  // Position: the first argmin over k < 128 of |bar_st + k T / 128 - start| (np.linspace(bar_st, bar_et, 128, endpoint=False)).  A
  // division by 128 is exact in binary and k T / 128 + bar_st < 2^33 has at most 40 significant bits, so the float64 values the
  // reference compares are the exact rationals: compare |k T - 128 d| in integers, d = start - bar_st in [0, T).
  const long long d128 = ((long long)start - bar_st) * 128;
  int k = (int)(d128 / T);                                        // <= 127
  const long long r0 = d128 - (long long)k * T;                   // distance to flag k (below or at), T - r0 to flag k + 1
  if (k < 127 && T - r0 < r0) ++k;                                // a tie keeps the first
  w[0] = 432 + k;
  // Velocity: searchsorted(linspace(2, 127, 64, dtype=int), v, 'right') - 1, bins 2 + (125 j) / 63; below 2 the index is -1: "Note
  // Velocity_-1" is unknown and becomes Note Velocity_63 (194), with an OOV line
  if (vel < 2) { w[1] = 194; ++oov; }
  else {
    int j = 63;
    while (j > 0 && 2 + (125 * j) / 63 > vel) --j;
    w[1] = 131 + j;
  }
  if (pitch >= 0 && pitch <= 127) w[2] = 3 + pitch;
  else { w[2] = -1; ++oov; }
  // Duration: the first argmin against step * (1 .. T / step), step = T / 128; an index above 127 (T no multiple of 128) is unknown
  // and becomes Note Duration_127, silently
  const int step = T / 128, m = T / step;
  const long long dur = (long long)end - start;
  int idx = 0;
  if (dur > step) {
    const long long q = dur / step;
    const int lo = (int)(q < m ? q : m) - 1;
    idx = lo;
    if (lo + 1 < m) {
      const long long dlo = dur - (long long)(lo + 1) * step, dhi = (long long)(lo + 2) * step - dur;
      if (dhi < dlo) idx = lo + 1;
    }
  }
  w[3] = 304 + (idx > 127 ? 127 : idx);
  return oov;
}

__global__ __launch_bounds__(TB) void encode_events_kernel(const int32_t* __restrict__ notes, const int32_t* __restrict__ n_notes,
                                                          const int32_t* __restrict__ params, const int32_t* __restrict__ slots,
                                                          const int32_t* __restrict__ n_slots, int32_t* __restrict__ words,
                                                          int32_t* __restrict__ length, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ status, int max_notes, int max_slots, int ld) {
  __shared__ unsigned long long key[MAX_UNITS];
  __shared__ int32_t pay[MAX_UNITS];
  __shared__ int32_t order[MAX_NOTES];   // order[r] = input index of the r-th note by (start, pitch, input index)
  __shared__ int wsum[4];
  __shared__ long long red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t* nt = notes + (int64_t)b * max_notes * 4;
  const int32_t* sl = slots + (int64_t)b * max_slots * 2;
  int32_t* out = words + (int64_t)b * ld;
  const int tpb = params[b * 5 + 0], num = params[b * 5 + 1], den = params[b * 5 + 2];
  const int NM = params[b * 5 + 3] > 0 ? params[b * 5 + 3] : 0;    // range(num_measures) of a negative number is empty
  const int inc = params[b * 5 + 4] != 0;
  const int n = n_notes[b], S = n_slots[b];
  int st = MH_ENCODE_OK, T = 0, cpb = 0;

  // encoder.py:30-31: ticks_per_bar = int(ticks_per_beat * (numerator / denominator * 4)); encoder_utils.py:201, :357: chords per bar =
  // int(ticks_per_bar / ticks_per_beat) * 2 - float64, the reference's operations in its order
  if (tpb <= 0 || num <= 0 || den <= 0) st = MH_ENCODE_BAD_TIMEBASE;
  else {
    const double x = __dmul_rn((double)tpb, __dmul_rn(__ddiv_rn((double)num, (double)den), 4.0));
    if (!(x < (double)(MAX_T + 1))) st = MH_ENCODE_BAD_TIMEBASE;
    else {
      T = (int)x;
      if (T < 128 || T > MAX_T) st = MH_ENCODE_BAD_TIMEBASE;      // int(T / 128) == 0: np.arange's step, ZeroDivisionError
      else {
        cpb = (int)__ddiv_rn((double)T, (double)tpb) * 2;         // T / tpb <= 2^24
        if (cpb <= 0) st = MH_ENCODE_BAD_TIMEBASE;
      }
    }
  }
  if (st == MH_ENCODE_OK) {
    if (n <= 0) st = MH_ENCODE_EMPTY;
    else if (S <= 0) st = MH_ENCODE_NO_CHORDS;
    else if (n > max_notes || n > MAX_NOTES || S > max_slots || S > MAX_SLOTS) st = MH_ENCODE_OVERFLOW;
    else if (S % cpb) st = MH_ENCODE_BAD_CHORDS;
    else if ((long long)NM + S + n > MAX_UNITS) st = MH_ENCODE_OVERFLOW;
  }

  long long n_events = 0, n_oov = 0;
  int W = 0;
  if (st == MH_ENCODE_OK) {                                        // uniform
    // ---- read_items: the notes by (start, pitch, input index)
    const int P1 = next_pow2(n);                                   // <= MAX_NOTES
    for (int r = tid; r < P1; r += TB) {
      key[r] = r < n ? ((unsigned long long)((uint32_t)nt[r * 4 + 0] ^ 0x80000000u) << 32) | ((uint32_t)nt[r * 4 + 2] ^ 0x80000000u) : KEY_NONE;
      pay[r] = r;                                                  // a real key equal to KEY_NONE still sorts before the padding: r < n
    }
    bitonic_sort(key, pay, P1);
    for (int r = tid; r < n; r += TB) order[r] = pay[r];           // < n
    __syncthreads();
    // ---- group_items: downbeats = arange(0, max_time + T, T) with max_time the end of the LAST sorted note; a note is kept when
    // it starts in [0, last downbeat)
    const long long stop = (long long)nt[order[n - 1] * 4 + 1] + T;
    const long long nd = stop > 0 ? (stop + T - 1) / T : 0;
    const long long last_db = nd >= 2 ? (nd - 1) * T : 0;          // nd < 2: no pair of downbeats, no note survives
    // ---- the units: measure i -> Bar at i T; chord slot s -> (Position, Chord) when it is a change that insert_chord_on_event
    // consumes; sorted note r -> its four events.  U <= MAX_UNITS
    const int U = NM + S + n, P2 = next_pow2(U);
    for (int u = tid; u < P2; u += TB) {
      unsigned long long kk = KEY_NONE;
      int32_t pp = INT_MAX - u;                                    // distinct; only ever compared among KEY_NONE entries
      if (u < NM) {
        kk = (unsigned long long)((long long)u * T + 0x80000000ll);
        pp = u * (S + 1);
      } else if (u < NM + S) {
        // detect_chord: slot s = bar * cpb + c is a change when c == 0 or its name differs from the previous slot's (the previous
        // change's name is the previous slot's name).  insert_chord_on_event pops it in the first measure i with position < i + 1 - inc,
        // which is i = bar + inc (the fraction is below 1), if that measure exists.
        const int s = u - NM, bar = s / cpb, c = s % cpb, m = bar + inc;
        if ((c == 0 || sl[s * 2] != sl[(s - 1) * 2]) && m < NM) {
          const double pos = __dadd_rn((double)bar, __ddiv_rn((double)c, (double)cpb));
          const long long t = (long long)__dadd_rn(__dmul_rn(pos, (double)T), (double)((long long)T * inc));   // < 2^35
          kk = (unsigned long long)(t + 0x80000000ll);
          pp = m * (S + 1) + 1 + s;                                // < 4096 * 1025 < NOTE_BASE
        }
      } else if (u < U) {
        const int r = u - NM - S;
        const int start = nt[order[r] * 4 + 0];
        if (start >= 0 && start < last_db) {
          kk = (unsigned long long)((long long)start + 0x80000000ll);
          pp = NOTE_BASE + r;
        }
      }
      key[u] = kk;
      pay[u] = pp;
    }
    bitonic_sort(key, pay, P2);
    // ---- expand the units in order.  Emitting units come first (their keys are below 2^36)
    for (int j0 = 0; j0 < U; j0 += TB) {
      const int j = j0 + tid;
      int32_t w[4] = {-1, -1, -1, -1};
      if (j < U && key[j] != KEY_NONE) {
        const int32_t p = pay[j];
        if (p >= NOTE_BASE) {
          const int32_t* q = nt + order[p - NOTE_BASE] * 4;        // p - NOTE_BASE < n
          const int start = q[0];
          n_oov += note_words(start, q[1], q[2], q[3], (long long)(start / T) * T, T, w);
          n_events += 4;
        } else {
          const int m = p / (S + 1), sub = p % (S + 1);
          if (sub == 0) {
            w[0] = 2;
            n_events += 1;
          } else {
            // the Position value int((chord_position - i + inc) * 128) + 1 in float64, as written; chord_position = bar + c / cpb
            const int s = sub - 1, bar = s / cpb, c = s % cpb;     // s < S
            const double pos = __dadd_rn((double)bar, __ddiv_rn((double)c, (double)cpb));
            const double f = __dmul_rn(__dadd_rn(__dsub_rn(pos, (double)m), (double)inc), 128.0);   // in [0, 128)
            const int v = (f >= 0.0 && f < 128.0) ? (int)f : -1;
            const int32_t tok = sl[s * 2 + 1];
            if (v >= 0) w[0] = 432 + v; else ++n_oov;
            if (tok >= 195 && tok <= 303) w[1] = tok; else ++n_oov;   // -1: the reference prints "OOV Chord_..." and writes no word
            n_events += 2;
          }
        }
      }
      const int cnt = (w[0] >= 0) + (w[1] >= 0) + (w[2] >= 0) + (w[3] >= 0);
      int total;
      int at = W + block_excl_scan(cnt, wsum, total);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (w[k] >= 0) {
          if (at < ld) out[at] = w[k];
          ++at;
        }
      W += total;
    }
    n_events = block_sum(n_events, red);
    n_oov = block_sum(n_oov, red);
    if (W + 1 > ld) st = MH_ENCODE_OVERFLOW;
  }
  __syncthreads();                                                 // the zero fill may overwrite what other threads wrote
  const int len = st == MH_ENCODE_OK ? W + 1 : 0;
  for (int j = len + tid; j < ld; j += TB) out[j] = 0;
  if (tid == 0) {
    if (len) out[len - 1] = 1;                                     // EOS; len <= ld
    length[b] = len;
    counts[b * 2 + 0] = st == MH_ENCODE_OK ? (int)n_events : 0;
    counts[b * 2 + 1] = st == MH_ENCODE_OK ? (int)n_oov : 0;
    status[b] = st;
  }
}

// ---- merge_and_mask.  chord(j) = 195 <= trg[j] <= 303.  The gathered pairs are (j - 1, j) per chord j, -1 wrapping to n - 1 as numpy's
// negative index does; removed are the indices of all pairs: keep(j) = !chord(j) && !chord(j + 1) && !(j == n - 1 && chord(0)).
struct MergeRow {
  const int32_t* trg;
  int n, sl;
};

__device__ __forceinline__ bool is_chord(const MergeRow& r, int j) { return r.trg[j] >= 195 && r.trg[j] <= 303; }   // 0 <= j < n
__device__ __forceinline__ bool is_kept(const MergeRow& r, int j) {
  return !is_chord(r, j) && !(j + 1 < r.n && is_chord(r, j + 1)) && !(j == r.n - 1 && is_chord(r, 0));
}

__device__ __forceinline__ MergeRow merge_row(const int32_t* src_len, const int32_t* words, const int32_t* lengths, const int32_t* status_in,
                                              int b, int S, int ld, int& st) {
  MergeRow r;
  r.trg = words + (int64_t)b * ld;
  st = status_in ? status_in[b] : MH_ENCODE_OK;
  const int n = lengths[b];
  r.n = st != MH_ENCODE_OK ? 0 : (n < 0 ? 0 : (n > ld ? ld : n));
  const int sl = src_len ? src_len[b] : S;
  r.sl = sl < 0 ? 0 : (sl > S ? S : sl);
  return r;
}

__global__ __launch_bounds__(TB) void merge_length_kernel(const int32_t* __restrict__ src_len, const int32_t* __restrict__ words,
                                                         const int32_t* __restrict__ lengths, const int32_t* __restrict__ status_in,
                                                         int32_t* __restrict__ length, int32_t* __restrict__ status, int S, int ld) {
  __shared__ long long red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int st;
  const MergeRow r = merge_row(src_len, words, lengths, status_in, b, S, ld, st);
  long long c = 0;
  for (int j = tid; j < r.n; j += TB) c += 2 * (int)is_chord(r, j) + (int)is_kept(r, j);
  c = block_sum(c, red);
  if (tid == 0) {
    length[b] = st == MH_ENCODE_OK ? (int)(r.sl + 1 + c) : 0;      // <= S + 1 + 2 ld
    status[b] = st;
  }
}

// offsets[b + 1] = sum of length[..b] while the sum fits cap; the rows behind that get length 0 and OVERFLOW
__global__ __launch_bounds__(TB) void merge_offsets_kernel(int32_t* __restrict__ length, int32_t* __restrict__ status,
                                                          int64_t* __restrict__ offsets, int B, int64_t cap) {
  __shared__ long long wtot[4];
  __shared__ long long red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long run = 0, fit = 0;
  if (tid == 0) offsets[0] = 0;
  for (int b0 = 0; b0 < B; b0 += TB) {
    const int b = b0 + tid;
    long long incl = b < B ? length[b] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += wtot[w];
    incl += run;
    run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    if (b < B) {
      offsets[b + 1] = incl;
      if (incl <= cap && incl > fit) fit = incl;
    }
  }
  fit = block_max(fit, red);                                       // also orders this block's writes of offsets before the reads below
  for (int b = tid; b < B; b += TB)
    if (offsets[b + 1] > cap) {
      offsets[b + 1] = fit;
      if (length[b] > 0) { length[b] = 0; status[b] = MH_ENCODE_OVERFLOW; }
    }
}

__global__ __launch_bounds__(TB) void merge_write_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ src_len,
                                                        const int32_t* __restrict__ words, const int32_t* __restrict__ lengths,
                                                        const int32_t* __restrict__ status_in, const int32_t* __restrict__ length,
                                                        const int64_t* __restrict__ offsets, int32_t* __restrict__ ids,
                                                        int32_t* __restrict__ mask, int S, int ld, int64_t cap) {
  __shared__ int wsum[4];
  __shared__ long long red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int st;
  const MergeRow r = merge_row(src_len, words, lengths, status_in, b, S, ld, st);
  const int64_t o = offsets[b];
  const int len = length[b];
  if (len <= 0 || o < 0 || o + len > cap) return;                  // uniform: a row that failed, or that the offsets kernel cut
  long long c = 0;
  for (int j = tid; j < r.n; j += TB) c += (int)is_chord(r, j);
  const int nch = (int)block_sum(c, red);
  const int head = r.sl + 2 * nch + 1;                             // src + pairs + EOS; head + kept == len
  for (int k = tid; k < r.sl; k += TB) ids[o + k] = src[(int64_t)b * S + k];
  if (tid == 0) ids[o + head - 1] = 1;
  for (int k = tid; k < len; k += TB) mask[o + k] = k >= head;
  int ch = 0, kp = 0;
  for (int j0 = 0; j0 < r.n; j0 += TB) {
    const int j = j0 + tid;
    const bool chord = j < r.n && is_chord(r, j), keep = j < r.n && is_kept(r, j);
    int tc, tk;
    const int ec = ch + block_excl_scan(chord, wsum, tc), ek = kp + block_excl_scan(keep, wsum, tk);
    if (chord) {                                                   // ec < nch
      ids[o + r.sl + 2 * ec] = r.trg[j == 0 ? r.n - 1 : j - 1];
      ids[o + r.sl + 2 * ec + 1] = r.trg[j];
    }
    if (keep && head + ek < len) ids[o + head + ek] = r.trg[j];
    ch += tc;
    kp += tk;
  }
}

}  // namespace

extern "C" int mh_encode_max_notes(void) { return MAX_NOTES; }
extern "C" int mh_encode_max_slots(void) { return MAX_SLOTS; }

extern "C" int mh_encode_events(const int32_t* notes, const int32_t* n_notes, const int32_t* params, const int32_t* chord_slots,
                                const int32_t* n_slots, int32_t* words, int32_t* length, int32_t* counts, int32_t* status, int B,
                                int max_notes, int max_slots, int ld, mh_stream_t stream) {
  MH_CHECK_ARG(notes && n_notes && params && chord_slots && n_slots && words && length && counts && status && B > 0 && max_notes > 0 &&
                   max_slots > 0 && ld > 0, "encode_events: bad arguments");
  MH_CHECK_ARG(ld <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "encode_events: rows of at most %d words (got ld = %d)", MAX_ROW, ld);
  MH_LAUNCH(encode_events_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, notes, n_notes, params, chord_slots, n_slots, words, length,
            counts, status, max_notes, max_slots, ld);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_merge_and_mask(const int32_t* src, const int32_t* src_len, const int32_t* words, const int32_t* lengths,
                                 const int32_t* status_in, int32_t* ids, int32_t* mask, int64_t* offsets, int32_t* length, int32_t* status,
                                 int B, int S, int ld, int64_t cap, mh_stream_t stream) {
  MH_CHECK_ARG(src && words && lengths && ids && mask && offsets && length && status && B > 0 && S > 0 && ld > 0 && cap > 0,
               "merge_and_mask: bad arguments");
  MH_CHECK_ARG(S <= MAX_ROW && ld <= MAX_ROW, "merge_and_mask: rows of at most %d tokens (got S = %d, ld = %d)", MAX_ROW, S, ld);
  MH_LAUNCH(merge_length_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, src_len, words, lengths, status_in, length, status, S, ld);
  MH_CHECK_LAUNCH();
  MH_LAUNCH(merge_offsets_kernel, dim3(1), dim3(TB), 0, (hipStream_t)stream, length, status, offsets, B, cap);
  MH_CHECK_LAUNCH();
  MH_LAUNCH(merge_write_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, src, src_len, words, lengths, status_in, length, offsets, ids,
            mask, S, ld, cap);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
