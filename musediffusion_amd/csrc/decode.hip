// Token rows -> restored note sequences -> notes and chord markers, on the device (the last row "next to the path").
// Reference: MuseDiffusion/utils/decode_util.py:192-199 split_meta_midi, :73-84 remove_padding, :85-142 restore_chord, :145-156
// validate_once; commu/preprocessor/encoder/encoder.py:71-97 decode, encoder_utils.py:370-497 word_to_event / write_midi (the part
// before the miditoolkit container is filled).  Conventions of batch.hip: one 256-thread block per row, the row in LDS (at most
// MH_BATCH_MAX_ROW tokens), scans by ballot + popcount, int32 in and out, asynchronous on the given stream, no allocation.
// Latency-bound integer work - no MFMA shape here.
//
// Who decides: every data-dependent decision (entry branch, where to splice, when the reference would raise) is a function of values
// all 256 threads hold alike - block-reduced counts and LDS contents read at uniform indices - so each thread evaluates the same scalar
// code and no broadcast is needed; the searches (last candidate position token of a bar) and the copies are spread over the block.
//
// Memory safety: every index into LDS is below n <= MAX_ROW by construction (commented where it is not obvious), every global write is
// guarded by its buffer's capacity, and a row whose mask, tokens or lengths make no sense gets a status, not a pointer.
#include "common.h"

namespace {

constexpr int TB = 256;
constexpr int MAX_ROW = 4096;   // == mh_batch_max_row() (batch.hip); the wrappers check it

// exclusive prefix sums of three flags per thread over the block; totals[k] = block total of flag k
__device__ __forceinline__ void block_excl_scan3(const int (&flag)[3], int (*wsum)[4], int (&excl)[3], int (&total)[3]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(flag[k] != 0);
    before[k] = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[k][wave] = __builtin_popcountll(m);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[k][w];
    total[k] = wsum[k][0] + wsum[k][1] + wsum[k][2] + wsum[k][3];
    excl[k] = base + before[k];
  }
  __syncthreads();
}

__device__ __forceinline__ int block_excl_scan1(int flag, int (*wsum)[4], int& total) {
  const int f[3] = {flag, 0, 0};
  int e[3], t[3];
  block_excl_scan3(f, wsum, e, t);
  total = t[0];
  return e[0];
}

// block-wide sum / max of one value per thread, returned to every thread
template <bool MAX>
__device__ __forceinline__ long long block_reduce(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long u = __shfl_xor(v, o, 64);
    v = MAX ? (u > v ? u : v) : v + u;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = MAX ? (red[w] > r ? red[w] : r) : r + red[w];
  __syncthreads();
  return r;
}

// split_meta_midi + remove_padding + restore_chord of row b.  restored[b, :restored_len[b]] = the sequence, the rest of the row 0;
// meta[b] = the first 11 tokens of the meta (0 where the meta is shorter); status[b] = mh_decode_status, restored_len 0 unless OK.
__global__ __launch_bounds__(TB) void restore_chord_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ input_mask,
                                                          int32_t* __restrict__ restored, int32_t* __restrict__ restored_len,
                                                          int32_t* __restrict__ meta, int32_t* __restrict__ status, int L, int ld_out) {
  __shared__ int32_t s[MAX_ROW];    // the note sequence, cut after its first EOS (branch "fewer": with the inserted Bars)
  __shared__ int32_t ci[MAX_ROW];   // the chord part of the meta: meta[11:]
  __shared__ int bars[MAX_ROW];     // indices of the Bar tokens of s, ascending
  __shared__ int wsum[3][4];
  __shared__ long long red[4];
  __shared__ int eos_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t* seq = tokens + (int64_t)b * L;
  const int32_t* msk = input_mask + (int64_t)b * L;
  int32_t* out = restored + (int64_t)b * ld_out;
  int st = MH_DECODE_OK, w = 0;

  // len_meta = L - sum(mask) (decode_util.py:194); a mask that is no 0 / 1 mask can put it anywhere: outside [0, L] is BAD_META
  long long part = 0;
  for (int j = tid; j < L; j += TB) part += msk[j];
  const long long lm = (long long)L - block_reduce<false>(part, red);
  if (lm < 0 || lm > L) st = MH_DECODE_BAD_META;
  const int len_meta = st == MH_DECODE_OK ? (int)lm : L;
  const int meta_len = len_meta >= 1 ? len_meta - 1 : L - 1;   // seq[:len_meta - 1]: with len_meta 0 the -1 counts from the end
  const int C = meta_len > 11 ? meta_len - 11 : 0;             // 11 + C <= L - 1
  if (tid < 11) meta[b * 11 + tid] = (st == MH_DECODE_OK && tid < meta_len) ? seq[tid] : 0;   // tid < meta_len <= L - 1

  // remove_padding: the notes are seq[len_meta : first EOS + 1]
  if (tid == 0) eos_s = L;
  __syncthreads();
  int first = L;
  for (int j = len_meta + tid; j < L; j += TB)
    if (seq[j] == 1 && j < first) first = j;
  if (first < L) atomicMin(&eos_s, first);
  __syncthreads();
  if (st == MH_DECODE_OK && eos_s >= L) st = MH_DECODE_NO_EOS;
  int n = st == MH_DECODE_OK ? eos_s - len_meta + 1 : 0;        // 1 <= n <= L - len_meta

  // the row, its Bars and the chord part into LDS; count the Bars and the 432s of the chord part (any index, as the reference does)
  int nb = 0;
  for (int j0 = 0; j0 < n; j0 += TB) {
    const int j = j0 + tid;
    int isbar = 0;
    if (j < n) {
      const int32_t v = seq[len_meta + j];
      s[j] = v;
      isbar = v == 2;
    }
    int total;
    const int r = nb + block_excl_scan1(isbar, wsum, total);
    if (isbar) bars[r] = j;                                      // r < n
    nb += total;
  }
  int c432 = 0;
  if (st == MH_DECODE_OK)
    for (int k = tid; k < C; k += TB) {
      const int32_t v = seq[11 + k];
      ci[k] = v;
      c432 += v == 432;
    }
  const int n432 = (int)block_reduce<false>(c432, red);         // also the barrier that publishes s, bars and ci

  // the three entry branches (decode_util.py:93-110); bars[0] / bars[1] of an empty / one-element list is the reference's IndexError
  int bc = 0;
  if (st == MH_DECODE_OK) {
    if (nb == n432) {
      if (nb == 0) st = MH_DECODE_REF_INDEXERROR;
    } else if (nb == n432 + 1) {
      if (nb < 2) st = MH_DECODE_REF_INDEXERROR;
      bc = 1;
    } else if (nb < n432) {
      // np.insert(seq, -1, 2) diff times: the missing Bars go in front of the last element (the EOS)
      const int diff = n432 - nb;
      if (n + diff > MAX_ROW) {
        st = MH_DECODE_OVERFLOW;                                 // only a len_meta of 0 gets here (else n + diff <= L)
      } else {
        const int32_t last = s[n - 1];
        __syncthreads();
        for (int k = tid; k < diff; k += TB) { s[n - 1 + k] = 2; bars[nb + k] = n - 1 + k; }
        if (tid == 0) s[n - 1 + diff] = last;
        __syncthreads();
        n += diff;
        nb = n432;
      }
    } else {
      st = MH_DECODE_RESTORE_FAILED;
    }
  }

  // w = length of new_seq so far; writes stop at ld_out, the length keeps counting so that the overflow is seen at the end
  auto append_seq = [&](int from, int to) {                      // s[from:to], 0 <= from, to <= n; empty when to <= from
    if (to <= from) return;
    for (int k = tid; k < to - from; k += TB)
      if (w + k < ld_out) out[w + k] = s[from + k];
    w += to - from;
  };
  auto append_pair = [&](int i) {                                // chord_info[i:i + 2], clamped by the end of the chord part
    const int cnt = C - i < 2 ? (C - i < 0 ? 0 : C - i) : 2;
    if (tid < cnt && w + tid < ld_out) out[w + tid] = ci[i + tid];
    w += cnt;
  };
  if (st == MH_DECODE_OK) {
    int last_idx = bars[bc];                                     // bc < nb in every surviving branch
    append_seq(0, last_idx + 1);
    append_pair(0);
    for (int i = 2; i < C; i += 2) {
      const int32_t v = ci[i];
      if (v == 432) {                                            // the next bar's chord: copy up to and including its Bar token
        if (bc + 1 >= nb) { st = MH_DECODE_REF_INDEXERROR; break; }   // bar_idx[bar_count + 1] past the end
        append_seq(last_idx + 1, bars[bc + 1] + 1);
        append_pair(i);
        ++bc;
        last_idx = bars[bc];
      } else {
        // a chord change at position token v inside bar bc: splice after the note whose position token is the last one below v in
        // the bar (candidate + 4; "+ 4" may run past the end, slices clamp), or right here when the bar has none
        const int lo = bars[bc], hi = bc != nb - 1 ? bars[bc + 1] : n;
        int p = -1;
        for (int j = lo + 1 + tid; j < hi; j += TB)
          if (s[j] >= 432 && s[j] < v) p = j;
        p = (int)block_reduce<true>(p, red);
        if (p >= 0) {
          append_seq(last_idx + 1, p + 4 < n ? p + 4 : n);
          last_idx = p + 3;                                      // may lie before the old last_idx, or at / past n - 1
        }
        append_pair(i);
      }
    }
    if (st == MH_DECODE_OK) append_seq(last_idx + 1, n);
    if (st == MH_DECODE_OK && w > ld_out) st = MH_DECODE_OVERFLOW;
  }
  __syncthreads();                                               // the zero fill may overwrite what other threads copied
  const int len = st == MH_DECODE_OK ? w : 0;
  for (int j = len + tid; j < ld_out; j += TB) out[j] = 0;
  if (tid == 0) { restored_len[b] = len; status[b] = st; }
}

// validate_once + word_to_event + write_midi's two passes of row b of restored [B, ld]
__global__ __launch_bounds__(TB) void decode_events_kernel(const int32_t* __restrict__ restored, const int32_t* __restrict__ restored_len,
                                                          const int32_t* __restrict__ meta, const int32_t* __restrict__ validate, int strict,
                                                          int32_t* __restrict__ notes, int32_t* __restrict__ chords, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ status, int ld, int max_notes, int max_chords) {
  __shared__ int32_t row[MAX_ROW];
  __shared__ int32_t comp[MAX_ROW];   // the row without the tokens outside 2..559
  __shared__ int wsum[3][4];
  __shared__ long long red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int st = status[b];
  int n = restored_len[b];
  n = n < 0 ? 0 : (n > ld ? ld : n);                             // ld <= MAX_ROW (wrapper)
  int n_notes = 0, n_chords = 0, n_oov = 0;
  if (st == MH_DECODE_OK) {                                      // uniform: st is one word per block
    const int32_t* seq = restored + (int64_t)b * ld;
    for (int j = tid; j < n; j += TB) row[j] = seq[j];
    __syncthreads();
    // validate_once over the WHOLE restored sequence (an EOS in the middle does not end it): a velocity token at idx <= n - 3 between
    // a position token (idx 0 looks at seq[-1], the last one) and (pitch, duration)
    int hit = 0;
    for (int i = tid; i + 2 < n; i += TB) {
      const int32_t t = row[i], prev = row[i == 0 ? n - 1 : i - 1];
      if (t >= 131 && t < 195 && prev >= 432 && prev < 560 && row[i + 1] >= 3 && row[i + 1] < 131 && row[i + 2] >= 304 && row[i + 2] < 432) hit = 1;
    }
    hit = (int)block_reduce<true>(hit, red);
    if (!hit) {
      st = MH_DECODE_ONCE_FAILED;
    } else if (strict) {
      // validate_rigidly stops at the first EOS, so mh_validate_tokens' walk over the cut sequence is the reference's walk.  Its -2
      // (position, velocity, EOS: seq[i + 3] past the cut) is the reference's IndexError only when nothing follows that EOS; with
      // tokens after it the reference reads them, finds the EOS where the pitch belongs and fails the ordinary way.
      const int eos = validate[b * 3 + 0], rigid = validate[b * 3 + 2];
      if (rigid != 1) st = (rigid == -2 && eos + 1 >= n) ? MH_DECODE_REF_INDEXERROR : MH_DECODE_STRICT_FAILED;
    }
    // the three meta tokens the decoder indexes tables with (a meta of fewer than 11 tokens has an empty chord part and never
    // survives restore_chord, so the first three slots are the meta's own here)
    const int32_t bpm = meta[b * 11 + 0], key = meta[b * 11 + 1], ts = meta[b * 11 + 2];
    if (st == MH_DECODE_OK && !(bpm >= 561 && bpm <= 600 && key >= 602 && key <= 625 && ts >= 627 && ts <= 630)) st = MH_DECODE_BAD_META;
    if (st == MH_DECODE_OK) {
      // word_to_event: drop what word2event does not know (EOS silently, the rest counted), keep the order
      int m = 0, oov = 0;
      for (int j0 = 0; j0 < n; j0 += TB) {
        const int j = j0 + tid;
        int keep = 0;
        int32_t t = 0;
        if (j < n) {
          t = row[j];
          keep = t >= 2 && t <= 559;
          oov += !keep && t != 1;
        }
        int total;
        const int r = m + block_excl_scan1(keep, wsum, total);
        if (keep) comp[r] = t;                                   // r < n
        m += total;
      }
      n_oov = (int)block_reduce<false>(oov, red);                // also publishes comp
      // write_midi: over range(m - 3) only.  Bar at i > 0; note = Position, Velocity, Note On, Duration; chord = Position, Chord
      const int beats = ts == 627 ? 4 : (ts == 630 ? 6 : 3);    // int(num / den * 4) of 4/4, 3/4, 6/8, 12/8
      const int tpb = 480 * beats, dstep = tpb / 128;
      int nbar = 0;
      for (int i0 = 0; i0 < m - 3; i0 += TB) {
        const int i = i0 + tid;
        int f[3] = {0, 0, 0};
        int32_t t = 0, t1 = 0, t2 = 0, t3 = 0;
        if (i < m - 3) {
          t = comp[i]; t1 = comp[i + 1]; t2 = comp[i + 2]; t3 = comp[i + 3];
          if (t == 2 && i > 0) f[0] = 1;
          else if (t >= 432) {                                   // comp holds 2..559 only
            if (t1 >= 131 && t1 < 195 && t2 >= 3 && t2 < 131 && t3 >= 304 && t3 < 432) f[1] = 1;
            else if (t1 >= 195 && t1 < 304) f[2] = 1;
          }
        }
        int e[3], tot[3];
        block_excl_scan3(f, wsum, e, tot);
        const int start = (nbar + e[0]) * tpb + ((t - 432) * tpb) / 128;   // np.linspace(bar start, bar end, 128, endpoint=False, dtype=int)
        if (f[1] && n_notes + e[1] < max_notes) {
          int32_t* o = notes + ((int64_t)b * max_notes + n_notes + e[1]) * 4;
          o[0] = start;
          o[1] = start + (t3 - 304 + 1) * dstep;                 // duration_bins = arange(dstep, tpb + 1, dstep)
          o[2] = t2 - 3;
          o[3] = 2 + (125 * (t1 - 131)) / 63;                    // np.linspace(2, 127, 64, dtype=int)
        }
        if (f[2] && n_chords + e[2] < max_chords) {
          int32_t* o = chords + ((int64_t)b * max_chords + n_chords + e[2]) * 2;
          o[0] = start;
          o[1] = t1;
        }
        nbar += tot[0]; n_notes += tot[1]; n_chords += tot[2];
      }
      if (n_notes > max_notes || n_chords > max_chords) st = MH_DECODE_OVERFLOW;
    }
  }
  if (tid == 0) {
    counts[b * 3 + 0] = n_notes; counts[b * 3 + 1] = n_chords; counts[b * 3 + 2] = n_oov;
    status[b] = st;
  }
}

}  // namespace

extern "C" int mh_restore_chord(const int32_t* tokens, const int32_t* input_mask, int32_t* restored, int32_t* restored_len, int32_t* meta,
                                int32_t* status, int B, int L, int ld_out, mh_stream_t stream) {
  MH_CHECK_ARG(tokens && input_mask && restored && restored_len && meta && status && B > 0 && L > 0 && ld_out > 0, "restore_chord: bad arguments");
  MH_CHECK_ARG(L <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "restore_chord: rows of at most %d tokens (got L = %d)", MAX_ROW, L);
  MH_LAUNCH(restore_chord_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, tokens, input_mask, restored, restored_len, meta, status, L, ld_out);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_decode_events(const int32_t* restored, const int32_t* restored_len, const int32_t* meta, const int32_t* validate, int strict,
                                int32_t* notes, int32_t* chords, int32_t* counts, int32_t* status, int B, int ld, int max_notes,
                                int max_chords, mh_stream_t stream) {
  MH_CHECK_ARG(restored && restored_len && meta && notes && chords && counts && status && B > 0 && ld > 0 && max_notes > 0 && max_chords > 0,
               "decode_events: bad arguments");
  MH_CHECK_ARG(!strict || validate, "decode_events: strict validation needs mh_validate_tokens' result for the restored rows");
  MH_CHECK_ARG(ld <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "decode_events: rows of at most %d tokens (got ld = %d)", MAX_ROW, ld);
  MH_LAUNCH(decode_events_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, restored, restored_len, meta, validate, strict, notes, chords,
            counts, status, ld, max_notes, max_chords);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
