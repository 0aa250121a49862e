// attn_stream.h - the streaming attention forward kernel, and how its instantiations are named.  Included by attention_stream.hip alone,
// which lists every instantiation once (the product's there, the debug library's remainder in attn_stream_dbg.h), so no kernel is
// instantiated in two objects.  The kernel has INTERNAL linkage: no other object names it.
#pragma once
#include "lds_dma.h"

namespace {

// Streaming attention (bf16, L a multiple of 256, >= 512 queries per block): persistent blocks of 16 waves, one
// 32-query tile per wave, K / V^T streamed through LDS in 256-key stages by LDS-DMA, double-buffered - the
// stage (or the next (batch, head)) after the current one is in flight while the current one is computed, so
// the HBM traffic is spread over the whole kernel instead of arriving as one burst per block before any MFMA
// can start (the LDS-resident attn_res_bf16_kernel, attention.hip, spends 10 of its 33 us per block in that burst at L = 512).
// V^T arrives in the "P-operand" key order (mh_gemm_qkv_vtperm): within every 16 keys the two middle groups of
// four are swapped, which is the order the S^T accumulator registers hold the probabilities in, so a stage
// is a straight 16-byte-granular copy (source-side XOR swizzle) and P feeds the P.V MFMA without a shuffle.
// DROP (training): attention-probability dropout (HF BertSelfAttention: softmax -> dropout -> . V).  The keep flags of the
// wave's 32 x 32 S^T sub-tile come from Philox (drop_keep_attn) and are written to `keep_bits` (lane-native words, common.h
// drop_word_index: one store per lane and 64-key tile) for the backward kernels - or, with bits_in, are read from it (mask injection).
// The softmax normaliser runs over the un-dropped probabilities; 1 / (1 - p) is folded into the final 1 / l.
// DROP: 0 = no dropout, 1 = generate the keep flags (Philox) and write the bit tensor, 2 = read the bit tensor (a pre-pass or a test
// wrote it)
// FULL: seq_len is a multiple of SK, so no stage or tile is partial - the key-bound compares (which hipcc if-converts into a compare
// + select per score of EVERY tile, a third of the tile's vector instructions) are compiled out
// KVNT: the K / V stage DMA with the nt cache policy (aux 2)
// PRE: the queries arrive pre-multiplied by scale x log2(e) (the QKV epilogue folds it in, mh_gemm_qkv_vtperm_qs), so the S^T
// accumulators are already in the log2 domain, and the running reference lives in their INITIAL value: the first MFMA of every S^T
// chain takes C = -reference (16 registers that change only when the reference moves), so a probability is exp2(accumulator) with
// no multiply-subtract per score - 32 of the ~170 vector instructions of a 64-key tile (the kernel is VALU-bound)
// ABL: timing-only ablations (tools/attn_bench.py --ablate; results are garbage): 1 no softmax vector work, 2 no S^T MFMAs, 4 no P.V MFMAs,
// 8 no LDS fragment reads, 16 no K / V stage DMA
// (which of these a problem gets, and why: stream_choose, attention_stream.hip)
// PRIO (A/B, mh_attention_set_stream 9 / 10): one static s_setprio 1 for the younger half of the block's waves (MI355X_MICROARCH.md, two waves
// per SIMD, item 4: the later-dispatched waves lose every issue arbitration at equal priority)
template <int DH, int NW = 16, int SK = 256, int DROP = 0, bool FULL = false, bool KVNT = false, bool PRE = false, int ABL = 0, int PRIO = 0>
__global__ __launch_bounds__(64 * NW) void attn_stream_bf16_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                                const bf16* __restrict__ VT, bf16* __restrict__ ctx,
                                                                int64_t ld_ctx, int L, int nh, int nbh, float scale_log2e,
                                                                int ctx_panel, float* __restrict__ lse2, int64_t qsB, int64_t qsH, int64_t qld,
                                                                const DropArgs drop, uint32_t* __restrict__ keep_bits, int bits_in) {
  // NW waves (one 32-query tile each), SK keys per stage.  16 x 256 fills a CU (128 KiB LDS, four waves per SIMD); 8 x 128
  // leaves half of the CU's registers and LDS for a GEMM block of the other graph branch
  constexpr int CH = DH / 8, RPB = 128 / DH, KROWB = DH * 2;
  constexpr int KS = DH / 16, DT = DH / 32;
  constexpr int KST = SK * KROWB, VT_BYTES = DH * 128;   // K stage bytes (= V stage bytes), V^T bytes per 64-key tile
  constexpr int PK = KST / 1024 / NW;                    // 1-KiB DMA pieces per wave per operand per stage
  constexpr int KRP = 1024 / KROWB;                      // K rows per piece
  static_assert(PK >= 1, "stage too small for the wave count");
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, lq = lane & 31;
  if constexpr (PRIO != 0) { if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1); }
  const int nqb = (L + 32 * NW - 1) / (32 * NW), nst = (L + SK - 1) / SK;   // the last stage / tile may be partial (L % 16 == 0)
  const int nitems = nbh * nqb;
  // XCD-aware item order (round 6): the query blocks of one (batch, head) (two at seq_len 1024, five at 2096) stream the same K / V^T
  // and should meet in one L2; at seq_len 512 (one block per (batch, head)) the order changes nothing
  const int bx = mh_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int my_items = (nitems - bx + (int)gridDim.x - 1) / (int)gridDim.x;
  const int total = my_items * nst;

  auto issue = [&](int g) {   // DMA stage g (of this block's flattened (item, stage) sequence) into buffer g & 1
    if constexpr ((ABL & 16) != 0) return;
    const int item = bx + (g / nst) * gridDim.x, st = g % nst;
    const int bh = item / nqb;
    const bf16* Kb = K + (int64_t)(bh / nh) * qsB + (int64_t)(bh % nh) * qsH + (int64_t)st * SK * qld;   // rows qld elements apart
    const bf16* Vb = VT + (int64_t)bh * DH * L + (int64_t)st * SK;
    char* kdst = smem_dyn + (g & 1) * (2 * KST);
    char* vdst = kdst + KST;
#pragma unroll
    for (int j = 0; j < PK; ++j) {
      const int p = wave + NW * j;
      const int row = p * KRP + lane / CH, pc = lane % CH;             // key within the stage, physical chunk
      const int lc = pc ^ ((row / RPB) & (CH - 1));
      int rsrc = row;                                                   // keys past the end: any valid row (their scores are masked)
      if (!FULL && st * SK + row >= L) rsrc = L - 1 - st * SK;
      mh_glds16<KVNT ? 2 : 0>(Kb + (int64_t)rsrc * qld + lc * 8, kdst + p * 1024);
    }
#pragma unroll
    for (int j = 0; j < PK; ++j) {
      const int p = wave + NW * j;
      const int t = p / (DH / 8), d = (p % (DH / 8)) * 8 + (lane >> 3), pc = lane & 7;
      const int lc = pc ^ ((d >> 1) & 7);
      int kc = t * 64 + lc * 8;                                         // 8 keys past the end: any valid chunk (finite values x P = 0)
      if (!FULL && st * SK + kc >= L) kc = L - 8 - st * SK;
      mh_glds16<KVNT ? 2 : 0>(Vb + (int64_t)d * L + kc, vdst + p * 1024);
    }
  };

  const int ksw0 = (lq / RPB) & (CH - 1), ksw1 = ((32 + lq) / RPB) & (CH - 1);
  bf16x8 qf[KS];
  f32x16 o[DT];
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 sinit;              // PRE: -reference (log2 domain) in every register
  bool first_tile = false;   // PRE: no reference yet (wave-uniform)
#pragma unroll
  for (int r = 0; r < 16; ++r) sinit[r] = 0.f;
  int q0 = 0;
  bool active = false;

  unsigned long long prof_acc[4] = {0, 0, 0, 0};
  if (total > 0) issue(0);
  for (int g = 0; g < total; ++g) {
    const int item = bx + (g / nst) * gridDim.x, st = g % nst;
    const int bh = item / nqb, qb = item % nqb;
    unsigned long long tp0 = 0, tp1 = 0, tp2 = 0;      // ABL bit 128: where a wave's time goes (clock stamps per stage, summed per wave)
    if constexpr ((ABL & 128) != 0) tp0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stage g (issued one stage ago) has landed
    if constexpr ((ABL & 128) != 0) tp1 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_barrier();                      // ... for every wave; buffer (g+1)&1 was released at the end of stage g-1
    if constexpr ((ABL & 128) != 0) tp2 = __builtin_amdgcn_s_memtime();
    if (g + 1 < total) issue(g + 1);
    if (st == 0) {
      q0 = qb * (32 * NW) + wave * 32;
      active = q0 < L;
      if (active) {
        const bf16* Qb = Q + (int64_t)(bh / nh) * qsB + (int64_t)(bh % nh) * qsH;
        int qr = q0 + lq; if (qr >= L) qr = L - 1;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if constexpr ((ABL & 64) != 0) { for (int j = 0; j < 8; ++j) qf[ks][j] = (bf16)(0.01f * (j + ks) + 0.001f * lq); }
          else qf[ks] = *reinterpret_cast<const bf16x8*>(Qb + (int64_t)qr * qld + 16 * ks + 8 * h);
        }
      }
#pragma unroll
      for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
      m_run = -INFINITY; l_run = 0.f;
      if constexpr (PRE) {
        m_run = 0.f; first_tile = true;
#pragma unroll
        for (int r = 0; r < 16; ++r) sinit[r] = 0.f;
      }
    }
    if (active) {
      const char* kbuf = smem_dyn + (g & 1) * (2 * KST);
      const char* vbuf = kbuf + KST;
      const int st_keys = L - st * SK;                                  // valid keys of this stage (>= 16)
      if constexpr (PRE) {
        // pre-scaled queries: 32-key sub-tiles, one S^T accumulator set live at a time (the 16 registers that freed hold the initial
        // accumulator = -reference).  The accumulators come out as score - reference in the log2 domain, so p = exp2(accumulator).
        for (int t2 = 0; t2 < SK / 32 && (FULL || t2 * 32 < st_keys); ++t2) {
          const int t = t2 >> 1, kt = t2 & 1;
          const char* kb = kbuf + t * (64 * KROWB);
          const char* vb = vbuf + t * VT_BYTES;
          const int sub_keys = FULL ? 32 : st_keys - t2 * 32;             // < 32 only in the sequence's last sub-tile
          f32x16 sa;
          {
            bf16x8 kf[KS];
            const int krow = 32 * kt + lq, ksw = kt ? ksw1 : ksw0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(kb + krow * KROWB + (((2 * ks + h) ^ ksw) << 4));
            // the chain's first MFMA reads its C operand from the initial-accumulator registers and writes the accumulator itself
            // (D != C): as a builtin hipcc copies the 16 registers first, which costs what the multiply-subtract did
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(sa) : "v"(kf[0]), "v"(qf[0]), "v"(sinit));
#pragma unroll
            for (int ks = 1; ks < KS; ++ks) sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], sa, 0, 0, 0);
          }
          if (!FULL && sub_keys < 32) {   // register r holds key (r & 3) + 8 (r >> 2) + 4 h of the sub-tile: mask the ones past the end
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if ((r & 3) + 8 * (r >> 2) + 4 * h >= sub_keys) sa[r] = -INFINITY;
          }
          // the row maximum of the 16 scores as ONE asm statement of v_max3 (fmaxf on MFMA outputs makes hipcc canonicalise every
          // input with a v_max first: 16 more instructions).  hipcc pads no hazard whose consumer sits inside an asm string: the
          // 12 wait states an 8-pass MFMA result needs before a VALU read open the string (cdna_hip_programming.md 5.7 item 2)
          float mx, mt1, mt2, mt3, mt4;
          asm volatile("s_nop 11\n\t"
                       "v_max3_f32 %0, %5, %6, %7\n\t"
                       "v_max3_f32 %1, %8, %9, %10\n\t"
                       "v_max3_f32 %2, %11, %12, %13\n\t"
                       "v_max3_f32 %3, %14, %15, %16\n\t"
                       "v_max3_f32 %4, %17, %18, %19\n\t"
                       "v_max3_f32 %0, %0, %1, %2\n\t"
                       "v_max3_f32 %1, %3, %4, %20\n\t"
                       "v_max_f32 %0, %0, %1"
                       : "=&v"(mx), "=&v"(mt1), "=&v"(mt2), "=&v"(mt3), "=&v"(mt4)
                       : "v"(sa[0]), "v"(sa[1]), "v"(sa[2]), "v"(sa[3]), "v"(sa[4]), "v"(sa[5]), "v"(sa[6]), "v"(sa[7]), "v"(sa[8]), "v"(sa[9]),
                         "v"(sa[10]), "v"(sa[11]), "v"(sa[12]), "v"(sa[13]), "v"(sa[14]), "v"(sa[15]));
          mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
          // the reference moves by `shift` when a row overshoots it by more than 2^8 (or on the item's first sub-tile, where it
          // becomes the sub-tile maximum): this sub-tile's accumulators, the running sum and the output are re-based
          if (first_tile || __builtin_amdgcn_ballot_w64(mx > 8.0f) != 0) {
            const float shift = first_tile ? mx : fmaxf(mx, 0.f);
            if (!first_tile) {
              const float alpha = __builtin_amdgcn_exp2f(-shift);
              l_run *= alpha;
#pragma unroll
              for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            }
            m_run += shift;
#pragma unroll
            for (int r = 0; r < 16; ++r) sa[r] -= shift;
#pragma unroll
            for (int r = 0; r < 16; ++r) sinit[r] = -m_run;
            first_tile = false;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) sa[r] = __builtin_amdgcn_exp2f(sa[r]);
          float ps4[4] = {sa[0], sa[1], sa[2], sa[3]};
#pragma unroll
          for (int r = 4; r < 16; ++r) ps4[r & 3] += sa[r];
          l_run += (ps4[0] + ps4[1]) + (ps4[2] + ps4[3]);
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (bf16)sa[8 * s2 + j];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              const int d = dt * 32 + lq;
              const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vb + d * 128 + (((2 * (2 * kt + s2) + h) ^ ((d >> 1) & 7)) << 4));
              o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
            }
          }
        }
      } else
      for (int t = 0; t < SK / 64 && (FULL || t * 64 < st_keys); ++t) {
        const char* kb = kbuf + t * (64 * KROWB);
        const char* vb = vbuf + t * VT_BYTES;
        const int tile_keys = FULL ? 64 : st_keys - t * 64;             // < 64 only in the sequence's last tile
        f32x16 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          bf16x8 kf[KS];
          const int krow = 32 * kt + lq, ksw = kt ? ksw1 : ksw0;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            if constexpr ((ABL & 8) != 0) kf[ks] = qf[(ks + 1) % KS];
            else kf[ks] = *reinterpret_cast<const bf16x8*>(kb + krow * KROWB + (((2 * ks + h) ^ ksw) << 4));
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kt][r] = (ABL & 2) ? 0.01f * r + (float)kf[0][r & 7] : 0.f;
          if constexpr ((ABL & 2) == 0) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s[kt], 0, 0, 0);
          }
        }
        if (!FULL && tile_keys < 64) {   // register r of sub-tile kt holds key 32 kt + (r & 3) + 8 (r >> 2) + 4 h: mask the ones past the end
#pragma unroll
          for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= tile_keys) s[kt][r] = -INFINITY;
        }
        if constexpr ((ABL & 1) == 0) {
        float mx4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; r += 4)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx4[e] = fmaxf(mx4[e], s[kt][r + e]);
        float mx = fmaxf(fmaxf(mx4[0], mx4[1]), fmaxf(mx4[2], mx4[3]));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // lazy rescale: the running reference m_run only moves when some row's tile maximum exceeds it by more than
        // 2^8 in the exponent domain (always on the first tile, where it is -inf); otherwise the probabilities are
        // taken against the stale reference (p <= 256, harmless in fp32 / bf16) and the 32 accumulator multiplies,
        // the exp of alpha and the l_run multiply are skipped.  The final o / l is unchanged up to rounding.
        if (__builtin_amdgcn_ballot_w64((mx - m_run) * scale_log2e > 8.0f) != 0) {
          const float m_new = fmaxf(m_run, mx);
          const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);
          l_run *= alpha;
          m_run = m_new;
#pragma unroll
          for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        }
        const float mb = m_run * scale_log2e;
        float ps4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(s[kt][r] * scale_log2e - mb);
            s[kt][r] = p;
            ps4[r & 3] += p;
          }
        l_run += (ps4[0] + ps4[1]) + (ps4[2] + ps4[3]);
        }
        if constexpr (DROP != 0) {
          const int nb32 = (L + 31) >> 5;
          const int64_t wi = drop_word_index(bh, nb32, q0 >> 5, (st * SK + t * 64) >> 6, lane);   // this lane's word of the 64-key tile
          uint32_t kw;
          if constexpr (DROP == 2) {
            kw = keep_bits[wi];
          } else {
            const int qc = q0 + lq < L ? q0 + lq : L - 1;
            const int kb = (st * SK + t * 64) >> 5;
            kw = drop_keep_attn(drop, bh, L, nb32, qc, kb, h);
            if (FULL || 32 < tile_keys) kw |= drop_keep_attn(drop, bh, L, nb32, qc, kb + 1, h) << 16;   // (wave-uniform)
            keep_bits[wi] = kw;
          }
#pragma unroll
          for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kt][r] = and_bits(s[kt][r], keep_mask(kw, 16 * kt + r));
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (bf16)s[kt][8 * s2 + j];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              const int d = dt * 32 + lq;
              bf16x8 vf;
              if constexpr ((ABL & 8) != 0) vf = qf[(dt + s2) % KS];
              else vf = *reinterpret_cast<const bf16x8*>(vb + d * 128 + (((2 * (2 * kt + s2) + h) ^ ((d >> 1) & 7)) << 4));
              if constexpr ((ABL & 4) != 0) asm volatile("" ::"v"(vf), "v"(pf));
              else o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
            }
          }
      }
      if (st == nst - 1) {   // last stage of this (batch, head): normalise and write the context rows
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const float inv = (DROP != 0 ? drop.rscale : 1.0f) / l_tot;
        const int qr = q0 + lq;
        {
          const int b = bh / nh, head = bh % nh;
          const int64_t tok = (int64_t)b * L + (qr < L ? qr : L - 1);
          // log2-domain log-sum-exp of the scaled scores: P[q][k] = exp2(s c - lse2[q]) (what the backward kernels re-create P from)
          if (lse2 && h == 0 && qr < L) lse2[(int64_t)bh * L + qr] = (PRE ? m_run : m_run * scale_log2e) + __builtin_amdgcn_logf(l_tot);
          // a lane holds 4 consecutive head-dim elements (8 B) of its query's row per group rg, its half-wave partner the next 4: one
          // v_permlane32_swap per dword and pair of groups gives every lane 16 contiguous bytes, so the row leaves in 2 instead of 4
          // stores per 32-column block (the store tail is issue-bound: cdna_hip_programming.md T21).  All lanes take part in the
          // swaps (queries past the end hold finite garbage and do not store); 8-byte stores where the context rows are not 16-B aligned
          const bool wide = ctx_panel || (ld_ctx % 8 == 0 && (reinterpret_cast<uintptr_t>(ctx) & 15) == 0);   // (wave-uniform)
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            bf16* dst = ctx_panel ? ctx + (((int64_t)(head * DT + dt)) * ld_ctx + tok) * 32 : ctx + tok * ld_ctx + head * DH + dt * 32;
            uint2 pk[4];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              bf16x4 v;
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = (bf16)(o[dt][rg * 4 + e] * inv);
              __builtin_memcpy(&pk[rg], &v, 8);
            }
            if constexpr ((ABL & 32) != 0) { if (pk[0].x == 0x12345678u) *reinterpret_cast<uint2*>(dst + 4 * h) = pk[0]; }
            else if (wide) {
#pragma unroll
              for (int k = 0; k < 4; k += 2) {
                uint2 a = pk[k], b = pk[k + 1];
                auto rx = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
                auto ry = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
                if (qr < L) *reinterpret_cast<uint4*>(dst + 8 * k + 8 * h) = uint4{rx[0], ry[0], rx[1], ry[1]};
              }
            } else if (qr < L) {
#pragma unroll
              for (int rg = 0; rg < 4; ++rg) *reinterpret_cast<uint2*>(dst + 8 * rg + 4 * h) = pk[rg];
            }
          }
        }
      }
    }
    mh_wait_lgkmcnt0_fence();
    if constexpr ((ABL & 128) != 0) {
      const unsigned long long tp3 = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_s_barrier();
      const unsigned long long tp4 = __builtin_amdgcn_s_memtime();
      prof_acc[0] += tp1 - tp0; prof_acc[1] += tp2 - tp1; prof_acc[2] += tp3 - tp2; prof_acc[3] += tp4 - tp3;
      if (g == total - 1 && lane == 0) {   // per (block, wave): DMA wait, top barrier, stage work, bottom barrier (shader clocks)
        unsigned long long* dstp = reinterpret_cast<unsigned long long*>(keep_bits) + ((size_t)blockIdx.x * NW + wave) * 4;
        dstp[0] = prof_acc[0]; dstp[1] = prof_acc[1]; dstp[2] = prof_acc[2]; dstp[3] = prof_acc[3];
      }
    } else
    __builtin_amdgcn_s_barrier();                      // every wave is done reading buffer g & 1
  }
}

// One instantiation, by the kernel's template arguments; of<...>() takes them as the kernel does, defaults included.  Everything a launch needs
// beside the pointer follows from these numbers.
struct StreamVariant {
  int dh, nw, sk, dropv;
  bool full, kvnt, pre;
  int abl, prio;
  template <int DH, int NW = 16, int SK = 256, int DROP = 0, bool FULL = false, bool KVNT = false, bool PRE = false, int ABL = 0, int PRIO = 0>
  static constexpr StreamVariant of() { return {DH, NW, SK, DROP, FULL, KVNT, PRE, ABL, PRIO}; }
  constexpr bool operator==(const StreamVariant& o) const {
    return dh == o.dh && nw == o.nw && sk == o.sk && dropv == o.dropv && full == o.full && kvnt == o.kvnt && pre == o.pre && abl == o.abl && prio == o.prio;
  }
  constexpr int lds_bytes() const { return 2 * 2 * sk * dh * 2; }   // two buffers of a K stage and a V^T stage, sk keys x dh bf16 each
  constexpr int block() const { return 64 * nw; }
  constexpr int queries() const { return 32 * nw; }                 // per (batch, head, query block) item: one 32-query tile per wave
  constexpr int blocks_per_cu() const { return 16 / nw; }           // a CU holds 16 of these waves (registers) and their 128 KiB of LDS
};
// every instantiation has the same function type, so the pointer cannot tell which one it is: an entry pairs it with its variant
using StreamKernel = decltype(&attn_stream_bf16_kernel<64>);
struct StreamEntry { StreamVariant v; StreamKernel kern; };
#define MH_STREAM_ENTRY(...) {StreamVariant::of<__VA_ARGS__>(), &attn_stream_bf16_kernel<__VA_ARGS__>}

}  // namespace
