// Grammar-constrained rounding (include/musehip_grammar.h): the best token sequence the decode path accepts, instead of an argmax per
// position that decode.hip may reject as a whole.  Not in the reference (run/sample.py:218-220 takes the argmax and decode_util.py
// drops what does not parse).  Two kernels:
//   class_argmax_kernel   vocab_argmax_kernel of rounding.hip (modes 1 and 2) that also keeps, per token, the best (score, first index)
//                         of up to seven contiguous token ranges.  The contraction is that kernel's, statement for statement - fp32 fmaf
//                         chains, contraction off, 64 tokens x the whole vocabulary per block, 64 x 64 LDS tiles - so slot 7 is its
//                         answer bit for bit; the [N, V] scores never exist in memory.
//   constrain_rows_kernel one wave per row: a Viterbi pass over the note region with the automaton of the header, the BAR count k across
//                         the 64 lanes, then the trace-back.  Latency-bound integer and fp32 work, about L dependent steps per row.
// Conventions of decode.hip: int32 rows of at most mh_batch_max_row() tokens, asynchronous on the given stream, no allocation.
//
// Who decides in constrain_rows_kernel: which states are reachable is kept as 64-bit masks over k that every lane holds alike (built
// from ballots, kernel arguments and values read at uniform indices), so every decision word is wave-uniform; the scores live one k
// per lane and a score of an unreachable state is never looked at.
//
// Memory safety: len_meta in [0, L) is part of the status, decided before the region is touched; every table index is
// (b L + position) 8 + slot with position < L and slot < 8; every LDS index is 3 t + w with t < n <= L, and the launch gives the
// block 24 L bytes; every global write is inside the row's outputs.
#include "common.h"
#include "../../include/musehip_grammar.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------------------ class winners
constexpr int TLD = 68;   // padded LDS row (floats), as rounding.hip
constexpr int NCLS = 7;   // caller-given ranges; slot 7 = the whole vocabulary

template <int MODE>  // 1: logits (argmax x.W + b)   2: distance logits (argmax -sqrt(distance), logits_mode 2)
__global__ __launch_bounds__(256) void class_argmax_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                           const float* __restrict__ aux, const mhg_classes cls,
                                                           float* __restrict__ cls_score, int32_t* __restrict__ cls_idx,
                                                           int64_t n_tokens, int E, int V) {
  __shared__ __attribute__((aligned(16))) float Xs[64 * TLD];
  __shared__ __attribute__((aligned(16))) float Ws[64 * TLD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * 64;
  const int ne = (E + 63) / 64;

  float best[4][NCLS + 1];
  int bidx[4][NCLS + 1];
  float xn[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int c = 0; c < NCLS; ++c) { best[a][c] = -INFINITY; bidx[a][c] = -1; }
    best[a][NCLS] = -INFINITY;
    bidx[a][NCLS] = 0;
  }

  for (int v0 = 0; v0 < V; v0 += 64) {
    float dot[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) dot[a][b] = 0.f;
    for (int ec = 0; ec < ne; ++ec) {
      const int e0 = ec * 64;
      __syncthreads();
      for (int i = tid; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        int64_t tok = n0 + r; if (tok >= n_tokens) tok = n_tokens - 1;
        int vr = v0 + r; if (vr >= V) vr = V - 1;
        const bool in = (e0 + c) < E;
        Xs[r * TLD + c] = in ? x[tok * E + e0 + c] : 0.f;
        Ws[r * TLD + c] = in ? table[(int64_t)vr * E + e0 + c] : 0.f;
      }
      __syncthreads();
      if (MODE != 1 && v0 == 0) {
        // |x_n|^2, accumulated once (first vocabulary tile): lanes split the chunk, xor-reduce over tx
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float v = Xs[(4 * ty + a) * TLD + tx + 16 * k];
            s += v * v;
          }
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
          xn[a] += s;
        }
      }
#pragma unroll 2
      for (int e = 0; e < 64; e += 4) {
        f32x4 xv[4], wv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xv[a] = *reinterpret_cast<const f32x4*>(Xs + (4 * ty + a) * TLD + e);
#pragma unroll
        for (int b = 0; b < 4; ++b) wv[b] = *reinterpret_cast<const f32x4*>(Ws + (tx + 16 * b) * TLD + e);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) dot[a][b] = fmaf(xv[a][k], wv[b][k], dot[a][b]);
      }
    }
    float score[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int v = v0 + tx + 16 * b;
      const float av = v < V ? aux[v] : 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (MODE == 2) {
          const float dist = (av + xn[a]) - 2.0f * dot[a][b];
          score[a][b] = -sqrtf(fmaxf(dist, 0.0f));
        } else {
          score[a][b] = dot[a][b] + av;
        }
        // slot 7, the whole vocabulary: vocab_argmax_kernel's update (increasing v per lane: keeps the first)
        if (v < V && score[a][b] > best[a][NCLS]) { best[a][NCLS] = score[a][b]; bidx[a][NCLS] = v; }
      }
    }
    // the classes: only those whose range meets this tile's 64 columns (a uniform test on kernel arguments)
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      const int lo = cls.lo[c], hi = cls.hi[c] < V ? cls.hi[c] : V;
      if (hi > v0 && lo < v0 + 64) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int v = v0 + tx + 16 * b;
          const bool in = v >= lo && v < hi;
#pragma unroll
          for (int a = 0; a < 4; ++a)
            if (in && score[a][b] > best[a][c]) { best[a][c] = score[a][b]; bidx[a][c] = v; }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float s8[NCLS + 1];
    int i8[NCLS + 1];
#pragma unroll
    for (int c = 0; c <= NCLS; ++c) {
      float s = best[a][c];
      int i = bidx[a][c];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const float so = __shfl_xor(s, off, 64);
        const int io = __shfl_xor(i, off, 64);
        // an index is valid only with a score above -inf, so (-inf, -1) never displaces anything
        if (so > s || (so == s && io < i)) { s = so; i = io; }
      }
      s8[c] = s;
      i8[c] = i;
    }
    const int64_t tok = n0 + 4 * ty + a;
    if (tx == 0 && tok < n_tokens) {
      f32x4* so = reinterpret_cast<f32x4*>(cls_score + tok * 8);
      so[0] = f32x4{s8[0], s8[1], s8[2], s8[3]};
      so[1] = f32x4{s8[4], s8[5], s8[6], s8[7]};
      int4* io = reinterpret_cast<int4*>(cls_idx + tok * 8);
      io[0] = make_int4(i8[0], i8[1], i8[2], i8[3]);
      io[1] = make_int4(i8[4], i8[5], i8[6], i8[7]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ row Viterbi
constexpr int MAX_ROW = 4096;   // == mh_batch_max_row() (batch.hip); the wrapper checks it
constexpr int MAX_K = 63;       // one BAR count per lane

__device__ __forceinline__ float lane_f(float v, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j)); }
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long all_if(unsigned bits, int c) { return (bits >> c) & 1u ? ~0ull : 0ull; }

enum { S_A0 = 0, S_B0 = 1, S_V = 2, S_P = 3, S_D = 4, S_END = 5 };

__global__ __launch_bounds__(64) void constrain_rows_kernel(const float* __restrict__ cls_score, const int32_t* __restrict__ cls_idx,
                                                           const int32_t* __restrict__ ids, const int32_t* __restrict__ mask,
                                                           const int32_t* __restrict__ bar_lo, const int32_t* __restrict__ bar_hi, int policy,
                                                           int32_t* __restrict__ tokens, int32_t* __restrict__ status,
                                                           float* __restrict__ path_score, int32_t* __restrict__ counts, int L) {
  // per position of the region three decision words over k (into V: B0 instead of A0; into B0: BAR instead of DURATION; into END: PAD
  // instead of EOS); the trace-back leaves the class it read in the first of them
  extern __shared__ unsigned long long dec[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t row = (int64_t)b * L;

  // ---- the status, from values every lane holds alike
  long long part = 0;
  for (int j = lane; j < L; j += 64) part += mask[row + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  const long long lm = (long long)L - part;
  int st = MHG_OK, len_meta = 0, lo = 0, hi = 0;
  if (lm < 0 || lm >= L) {
    st = MHG_BAD_MASK;
  } else {
    len_meta = (int)lm;
    if (bar_lo) {
      lo = bar_lo[b];
      hi = bar_hi[b];
    } else {
      const int meta_end = len_meta >= 1 ? len_meta - 1 : L - 1;   // ids[11 : len_meta - 1]: with len_meta 0 the -1 counts from the end
      int c432 = 0;
      for (int j = 11 + lane; j < meta_end; j += 64) c432 += ids[row + j] == 432;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c432 += __shfl_xor(c432, o, 64);
      if (c432 == 0) st = MHG_NO_CHORDS;
      lo = policy == MHG_BARS_DECODABLE ? 0 : c432;
      hi = policy == MHG_BARS_DECODABLE ? c432 + 1 : c432;
    }
    if (st == MHG_OK && hi > MAX_K) st = MHG_TOO_MANY_BARS;
    if (st == MHG_OK && (lo < 0 || lo > hi)) st = MHG_BAD_BOUNDS;
  }
  st = __builtin_amdgcn_readfirstlane(st);
  len_meta = __builtin_amdgcn_readfirstlane(len_meta);
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  const int n = L - len_meta;                                      // 1 <= n <= L when st == MHG_OK

  int bars = 0, notes = 0, through_eos = 0;
  float total = 0.f;
  if (st == MHG_OK) {                                              // uniform
    const unsigned long long kmask = hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1ull;       // 0 <= hi <= 63
    const unsigned long long want = kmask & ~((1ull << lo) - 1ull);                      // 0 <= lo <= hi
    // reachable (state, k) as masks over k, and this lane's score of each state at k = lane
    unsigned long long rA0 = 1ull, rB0 = 0, rV = 0, rP = 0, rD = 0, rE = 0;
    float sA0 = 0.f, sB0 = 0.f, sV = 0.f, sP = 0.f, sD = 0.f, sE = 0.f;
    bool nonfinite = false;
    for (int t0 = 0; t0 < n; t0 += 64) {
      // 64 positions at once, one per lane: 32 B of scores and 32 B of indices each
      float sc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      unsigned avail = 0;
      bool bad = false;
      if (t0 + lane < n) {
        const int64_t at = (row + len_meta + t0 + lane) * 8;
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(cls_score + at), s1 = *reinterpret_cast<const f32x4*>(cls_score + at + 4);
        const int4 i0 = *reinterpret_cast<const int4*>(cls_idx + at), i1 = *reinterpret_cast<const int4*>(cls_idx + at + 4);
        sc[0] = s0[0]; sc[1] = s0[1]; sc[2] = s0[2]; sc[3] = s0[3]; sc[4] = s1[0]; sc[5] = s1[1]; sc[6] = s1[2];
        const int id[7] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z};
#pragma unroll
        for (int c = 0; c < NCLS; ++c) {
          avail |= (id[c] >= 0 ? 1u : 0u) << c;
          bad |= !(sc[c] < INFINITY);                              // NaN or +inf
        }
      }
      nonfinite |= __builtin_amdgcn_ballot_w64(bad) != 0;
      const int m = n - t0 < 64 ? n - t0 : 64;
      for (int j = 0; j < m; ++j) {
        const unsigned av = __builtin_amdgcn_readlane(avail, j);
        const float pPAD = lane_f(sc[MHG_PAD], j), pEOS = lane_f(sc[MHG_EOS], j), pBAR = lane_f(sc[MHG_BAR], j),
                    pPIT = lane_f(sc[MHG_PITCH], j), pVEL = lane_f(sc[MHG_VELOCITY], j), pDUR = lane_f(sc[MHG_DURATION], j),
                    pPOS = lane_f(sc[MHG_POSITION], j);
        const unsigned long long mBAR = all_if(av, MHG_BAR);
        // the scores one BAR ago come from the lane below; lane 0 has no such predecessor (its mask bit is 0)
        const float upA = __shfl_up(sA0, 1, 64), upB = __shfl_up(sB0, 1, 64);
        // into V: A0 before B0
        const unsigned long long v1 = rA0 & all_if(av, MHG_POSITION), v2 = rB0 & all_if(av, MHG_POSITION);
        const float fv1 = sA0 + pPOS, fv2 = sB0 + pPOS;
        const unsigned long long dV = v2 & (~v1 | __builtin_amdgcn_ballot_w64(fv2 > fv1));
        // into B0: DURATION before BAR
        const unsigned long long b1 = rD & all_if(av, MHG_DURATION), b2 = (rB0 << 1) & kmask & mBAR;
        const float fb1 = sD + pDUR, fb2 = upB + pBAR;
        const unsigned long long dB = b2 & (~b1 | __builtin_amdgcn_ballot_w64(fb2 > fb1));
        // into END: EOS before PAD
        const unsigned long long e1 = rB0 & all_if(av, MHG_EOS), e2 = rE & all_if(av, MHG_PAD);
        const float fe1 = sB0 + pEOS, fe2 = sE + pPAD;
        const unsigned long long dE = e2 & (~e1 | __builtin_amdgcn_ballot_w64(fe2 > fe1));
        const float nA0 = upA + pBAR, nP = sV + pVEL, nD = sP + pPIT;
        const unsigned long long nrA0 = (rA0 << 1) & kmask & mBAR, nrP = rV & all_if(av, MHG_VELOCITY), nrD = rP & all_if(av, MHG_PITCH);
        sV = (dV >> lane) & 1ull ? fv2 : fv1;
        sB0 = (dB >> lane) & 1ull ? fb2 : fb1;
        sE = (dE >> lane) & 1ull ? fe2 : fe1;
        sA0 = nA0; sP = nP; sD = nD;
        rV = v1 | v2; rB0 = b1 | b2; rE = e1 | e2;
        rA0 = nrA0; rP = nrP; rD = nrD;
        if (lane < 3) dec[3 * (t0 + j) + lane] = lane == 0 ? dV : (lane == 1 ? dB : dE);
      }
    }
    const unsigned long long fin = rE & want;
    if (nonfinite) st = MHG_NONFINITE;
    else if (fin == 0) st = MHG_NO_ROOM;
    __syncthreads();                                               // the decision words are read at uniform addresses below
    if (st == MHG_OK) {
      // the smallest k in [lo, hi] with the maximum score
      int kb = -1;
      for (int k = lo; k <= hi; ++k)
        if ((fin >> k) & 1ull) {
          const float v = lane_f(sE, k);
          if (kb < 0 || v > total) { kb = k; total = v; }
        }
      bars = kb;
      // the trace-back: everything is uniform
      int state = S_END, k = kb;
      for (int t = n - 1; t >= 0; --t) {
        int c;
        if (state == S_END) {
          if ((uniform64(dec[3 * t + 2]) >> k) & 1ull) { c = MHG_PAD; } else { c = MHG_EOS; state = S_B0; through_eos = t + 1; }
        } else if (state == S_B0) {
          if ((uniform64(dec[3 * t + 1]) >> k) & 1ull) { c = MHG_BAR; --k; } else { c = MHG_DURATION; state = S_D; ++notes; }
        } else if (state == S_D) {
          c = MHG_PITCH; state = S_P;
        } else if (state == S_P) {
          c = MHG_VELOCITY; state = S_V;
        } else if (state == S_V) {
          c = MHG_POSITION;
          state = (uniform64(dec[3 * t]) >> k) & 1ull ? S_B0 : S_A0;
        } else {
          c = MHG_BAR; --k;
        }
        if (lane == 0) dec[3 * t] = (unsigned long long)c;
      }
    }
  } else {
    __syncthreads();
  }
  __syncthreads();                                                 // the classes of the path are read by every lane
  const bool ok = st == MHG_OK;
  for (int pos = lane; pos < L; pos += 64) {
    const int c = ok && pos >= len_meta ? (int)dec[3 * (pos - len_meta)] : MHG_ANY;
    tokens[row + pos] = cls_idx[(row + pos) * 8 + c];
  }
  if (lane == 0) {
    status[b] = st;
    path_score[b] = ok ? total : 0.f;
    counts[b * 3 + 0] = ok ? bars : 0;
    counts[b * 3 + 1] = ok ? notes : 0;
    counts[b * 3 + 2] = ok ? through_eos : 0;
  }
}

}  // namespace

extern "C" int mhg_note_classes(mhg_classes* out) {
  MH_CHECK_ARG(out, "note_classes: null pointer");
  const int lo[NCLS] = {0, 1, 2, 3, 131, 304, 432}, hi[NCLS] = {1, 2, 3, 131, 195, 432, 560};
  for (int c = 0; c < NCLS; ++c) { out->lo[c] = lo[c]; out->hi[c] = hi[c]; }
  return MH_OK;
}

extern "C" int mhg_class_argmax(const float* x, const float* table, const float* aux, const mhg_classes* classes, float* cls_score,
                                int32_t* cls_idx, int64_t n_tokens, int E, int V, int mode, mh_stream_t stream) {
  MH_CHECK_ARG(x && table && aux && classes && cls_score && cls_idx, "class_argmax: null pointer");
  MH_CHECK_ARG(n_tokens > 0 && E > 0 && V > 0, "class_argmax: bad shape");
  MH_CHECK_ARG(mode == 1 || mode == 2, "class_argmax: mode 1 (logits) or 2 (distance logits), got %d", mode);
  MH_CHECK_ARG((n_tokens + 63) / 64 <= 0x7fffffff, "class_argmax: too many tokens");
  mhg_classes cls = *classes;
  for (int c = 0; c < NCLS; ++c)
    if (cls.lo[c] < 0) cls.lo[c] = 0;                               // only the part inside [0, V) counts; the kernel caps hi
  const dim3 grid((unsigned)((n_tokens + 63) / 64));
  if (mode == 1)
    MH_LAUNCH((class_argmax_kernel<1>), grid, dim3(256), 0, (hipStream_t)stream, x, table, aux, cls, cls_score, cls_idx, n_tokens, E, V);
  else
    MH_LAUNCH((class_argmax_kernel<2>), grid, dim3(256), 0, (hipStream_t)stream, x, table, aux, cls, cls_score, cls_idx, n_tokens, E, V);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" size_t mhg_constrain_workspace_bytes(int B, int L) {
  (void)B; (void)L;
  return 0;                                                         // the decision words live in LDS
}

extern "C" int mhg_constrain_rows(const float* cls_score, const int32_t* cls_idx, const int32_t* ids, const int32_t* mask,
                                  const int32_t* bar_lo, const int32_t* bar_hi, int policy, int32_t* tokens, int32_t* status,
                                  float* path_score, int32_t* counts, void* workspace, size_t workspace_bytes, int B, int L,
                                  mh_stream_t stream) {
  MH_CHECK_ARG(cls_score && cls_idx && ids && mask && tokens && status && path_score && counts && B > 0 && L > 0,
               "constrain_rows: bad arguments (a NULL pointer, B < 1 or L < 1)");
  MH_CHECK_ARG(L <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "constrain_rows: rows of at most %d tokens (got L = %d)", MAX_ROW, L);
  MH_CHECK_ARG((bar_lo != nullptr) == (bar_hi != nullptr), "constrain_rows: bar_lo and bar_hi come together");
  MH_CHECK_ARG(policy == MHG_BARS_EXACT || policy == MHG_BARS_DECODABLE, "constrain_rows: unknown policy %d", policy);
  MH_CHECK_ARG(workspace_bytes >= mhg_constrain_workspace_bytes(B, L) && (workspace || mhg_constrain_workspace_bytes(B, L) == 0),
               "constrain_rows: the workspace is too small");
  const size_t lds = (size_t)L * 3 * sizeof(unsigned long long);    // <= 96 KiB
  const int rc = mh_allow_dynamic_lds(reinterpret_cast<const void*>(constrain_rows_kernel), (size_t)MAX_ROW * 3 * sizeof(unsigned long long));
  if (rc != MH_OK) return rc;
  MH_LAUNCH(constrain_rows_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, cls_score, cls_idx, ids, mask, bar_lo, bar_hi, policy, tokens,
            status, path_score, counts, L);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
