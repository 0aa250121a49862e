// gemm_big.h - the bf16 big-tile kernel and its launcher.  Included by the gemm_big_*.hip objects, each of which instantiates
// launch_big<Cfg, EPI> for its tile configurations and nothing else (no kernel is instantiated in two objects), and by gemm_strip.hip for the
// DMA helpers.  The kernel and its device helpers keep INTERNAL linkage, as they had inside gemm.hip (no other object names them): with
// external linkage the LDS ring of a kernel instantiation becomes a linkonce symbol that the optimiser has to keep, and the "no DMA" timing
// ablations of the debug library (DBG bit 0), whose ring is never written, would allocate the LDS they run without today.
#pragma once
#include "gemm_args.h"

namespace mhgemm __attribute__((visibility("hidden"))) {
namespace {   // the kernel and its device helpers: internal linkage, as inside gemm.hip (see above)

// =====================================================================================================
// bf16 "big tile" kernels (the throughput path).  The kernel above is latency-bound at the denoiser's
// shapes (K = 512: eight K-steps, one tile of prefetch): rocprof showed ~14 us per 128x128 tile against
// 1.7 us of MFMA time.  These are built around keeping loads in flight:
//   * block tile BM x BN, WM x WN waves, each wave (BM/WM) x (BN/WN) = TI x TJ MFMA tiles of 16x16x32;
//     K-step 32; NST-stage LDS ring filled by global_load_lds_dwordx4 (one 1-KiB DMA piece = 16 rows x 64 B),
//     counted `s_waitcnt vmcnt(pieces x stages-in-flight)` + raw s_barrier so that younger stages stay in
//     flight ACROSS the barrier (a __syncthreads() would drain them).
//   * 64-B LDS rows, chunk c of row r stored at c ^ G[(r>>2)&3], G = {0,2,3,1}: every 16-lane group of a
//     ds_read_b128 fragment read hits 16 distinct 16-B slots (SQ_LDS_BANK_CONFLICT = 0); the DMA writes LDS
//     linearly, so the swizzle is applied to the per-lane global SOURCE address.
//   * the MFMA is issued with the operands SWAPPED (D = W_tile . A_tile^T) and the W rows of each 64-column
//     group are dealt to the MFMA input rows as 32(jj>>1) + 8(p>>2) + 4(jj&1) + (p&3): a lane then owns 8
//     CONSECUTIVE output columns of one row per (group, half), so bias / activation / residual / LayerNorm /
//     stores work straight from the accumulators with 16-byte accesses - no LDS round trip.
//     (V^T of the QKV projection wants consecutive TOKENS per lane instead: those waves issue the MFMA
//     un-swapped with the plain row order.)
//   * operands row-major or K32-panel (runtime strides only).
// Configurations:  Std 256x128 / 4 waves / 3 stages (72 KiB: two blocks per CU);  Wide 256x256 / 8 waves /
// 4 stages (128 KiB, 1.5x fewer DMA bytes per flop);  Row 128x512 / 8 waves / 3 stages (120 KiB): one block
// owns complete rows of an N = 512 output, which lets bias + residual + LayerNorm run in the epilogue.
// one DMA stage (K-step kt) of a tile into ring slot kt % NST: PA + PW 1-KiB pieces per wave
// the LayerNorm epilogue's residual rows are read once, by this block: non-temporal loads (same-box A/B of two builds: -0.6 % step time)
#ifndef MH_EPI3_RES_NT
#define MH_EPI3_RES_NT 1
#endif
// cache policy of the full-row (ping-pong) tile's A-operand DMA: nt (aux 2) - its rows are read by exactly one block, once, and
// should not displace the weight matrix every block re-reads from L2 (same-box A/B of two builds: -1.6 % step time; 0 = default policy)
#ifndef MH_PP_A_AUX
#define MH_PP_A_AUX 2
#endif
// DBG bit 16384 kernels (K32-panel operands only): the stage DMA as `buffer_load_dwordx4 ... lds` - ONE per-lane byte offset per operand for the
// whole kernel (a lane's chunk of its piece), the tile's base in a buffer descriptor (scalar registers), the K step as the instruction's
// scalar offset and a wave's consecutive pieces (16 rows x 64 B apart) as its immediate offset: no vector instruction per piece, where the
// `global_load_lds` form spends two 64-bit vector adds on every piece of every K step.  Rows beyond M / N are not clamped: inside the buffer they
// read other rows (their outputs are never stored), beyond it the descriptor's bound makes them zeros.
struct BufDma {
  __amdgpu_buffer_rsrc_t ra, rw;   // tile bases: A rows tm0.., W rows tn0.. of panel 0
  int va, vw;                      // this lane's byte offset inside its first piece's rows
  int ka, kw;                      // bytes per K32 panel
};
template <int J, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (J < N) { f(std::integral_constant<int, J>{}); static_for<J + 1, N>(f); }
}
template <class C>
__device__ __forceinline__ void issue_stage_buf(const char* smem, const BufDma& b, const int (&ldsA)[C::PA], const int (&ldsW)[C::PW], int kt) {
  char* base = const_cast<char*>(smem) + (kt % C::NST) * C::STAGE;
  constexpr int AUX_A = C::PP ? MH_PP_A_AUX : 0;     // (the full-row tile's A rows: nt, as in issue_stage)
  static_for<0, C::PA>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    // (the instruction's immediate offset advances the LDS address as well as the buffer address: every piece names the FIRST piece's slot)
    mh_buf_lds16<j * 1024, AUX_A>(b.ra, base + ldsA[0], b.va, kt * b.ka);
  });
  static_for<0, C::PW>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    mh_buf_lds16<j * 1024>(b.rw, base + C::BM * 64 + ldsW[0], b.vw, kt * b.kw);
  });
}

template <class C, int DBG>
__device__ __forceinline__ void issue_stage(const char* smem, const char* const (&srcA)[C::PA], const char* const (&srcW)[C::PW],
                                            const int (&ldsA)[C::PA], const int (&ldsW)[C::PW], int kt, int64_t kstepA,
                                            int64_t kstepW) {
  if constexpr ((DBG & 1) != 0) return;
  char* base = const_cast<char*>(smem) + (kt % C::NST) * C::STAGE;
#pragma unroll
  for (int j = 0; j < C::PA; ++j) {
    mh_glds16<C::PP ? MH_PP_A_AUX : 0>(srcA[j] + kt * kstepA, base + ldsA[j]);
  }
  if constexpr ((DBG & 4096) != 0) return;   // timing-only ablation: the W pieces are not issued (what their issue costs the loop)
#pragma unroll
  for (int j = 0; j < C::PW; ++j)
    mh_glds16(srcW[j] + kt * kstepW, base + C::BM * 64 + ldsW[j]);
}

// Main loop.  Fragments of K-step kt live in registers while its MFMAs run; the fragments of kt+1 are read
// from LDS underneath them (W into a second register set up front, the A row-fragment i into its own
// registers right after the last MFMA that uses it), so neither the LDS latency nor its bandwidth
// (12 KiB per wave per K-step) sits between two MFMA phases.  All NST ring slots hold DMA stages: slot
// kt % NST is refilled with stage kt + NST as soon as the barrier says every wave has read stage kt out of it.
// `pre`: 0 = issue the first stages here; 1 = they were issued before the previous tile's epilogue: drain everything (stores
// included); 2 = the same, and that epilogue issued exactly NSTORE stores per wave (a full tile): the waits for the prefetched
// stages count the stores as younger operations instead of waiting for them, so the stores drain under this tile's first K-steps.
template <class C, bool SWAP, int DBG, int NSTORE = 0>
__device__ __forceinline__ void big_mainloop(f32x4 (&acc)[C::TI][C::TJ], const char* smem, const char* const (&srcA)[C::PA],
                                             const char* const (&srcW)[C::PW], const int (&ldsA)[C::PA], const int (&ldsW)[C::PW],
                                             int nk, int a_off, const int (&b_offs)[C::TJ], int64_t kstepA, int64_t kstepW,
                                             int pre, unsigned* prof = nullptr, const BufDma* bd = nullptr) {
  constexpr int TI = C::TI, TJ = C::TJ;
  constexpr int NPIECES = (DBG & 4096) != 0 ? C::PA : C::PIECES;   // (ablation 4096: only the A pieces are issued)
  // DBG bit 4 (tools/gemm_bench.py --dbg 28): per-wave shader-clock totals of the three phases of a K-step
  unsigned long long pt_wait = 0, pt_bar = 0, pt_work = 0, pt0 = 0, pt1 = 0;
  auto tick = [&]() -> unsigned long long { if constexpr ((DBG & 16) != 0) return __builtin_amdgcn_s_memtime(); else return 0ull; };
  auto issue = [&](int kt) {
    if constexpr ((DBG & 16384) != 0) issue_stage_buf<C>(smem, *bd, ldsA, ldsW, kt);
    else issue_stage<C, DBG>(smem, srcA, srcW, ldsA, ldsW, kt, kstepA, kstepW);
  };
  auto read_frag = [&](const char* p) -> bf16x8 {
    if constexpr ((DBG & 8) != 0) { bf16x8 v; asm volatile("" : "=v"(v)); return v; }   // ablation: no LDS reads
    else return *reinterpret_cast<const bf16x8*>(p);
  };
  unsigned long long pc0 = 0, pr0 = 0;
  if constexpr ((DBG & 16) != 0) { pc0 = __builtin_amdgcn_s_memtime(); pr0 = __builtin_amdgcn_s_memrealtime(); }
  const int npro = nk < C::NST ? nk : C::NST;
  constexpr bool COUNTED = NSTORE > 0 && (C::NST - 1) * NPIECES + NSTORE <= 63;
  if (pre == 2 && COUNTED) {
    mh_wait_stages<NPIECES, COUNTED ? NSTORE : 0>(npro - 1);   // stage 0 landed; stages 1.. and the stores stay in flight
  } else if (pre) {   // the stages were issued before the previous tile's epilogue, whose stores share the counter: drain all
    mh_wait_vmcnt<0>();
  } else {
    for (int st = 0; st < npro; ++st) issue(st);
    mh_wait_stages<NPIECES>(npro - 1);
  }
  __builtin_amdgcn_s_barrier();
  bf16x8 a[TI], b[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) b[j] = read_frag(smem + C::BM * 64 + b_offs[j]);
#pragma unroll
  for (int i = 0; i < TI; ++i) a[i] = read_frag(smem + a_off + i * (16 * 64));
  auto mfma_row = [&](int i) {
    if constexpr ((DBG & 2) != 0) {
      asm volatile("" ::"v"(a[i]));
#pragma unroll
      for (int j = 0; j < TJ; ++j) asm volatile("" ::"v"(b[j]));
    } else {
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        if constexpr (SWAP) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  };
  // One K step.  (Two forms of it were built and measured out in round 5 - profiles/r05_ab_nulls.txt: the loop unrolled by the ring depth so
  // that every fragment read is `base + immediate`: +20 % per step, four copies of a K step do not fit the instruction cache; the next step's
  // W fragments into a second register set at the head of the step: +0.9 %, 16 registers and 8 moves per step.)
  auto kstep = [&](int kt) {
    const char* As = smem + ((kt + 1) % C::NST) * C::STAGE;
    const char* Ws = As + C::BM * 64;
    // stage kt+1 must have landed (stages kt+2 .. kt+NST-1 stay in flight across the barrier); this wave's
    // reads of stage kt were issued a whole MFMA phase ago, so the lgkmcnt wait is free
    const int younger = nk - 2 - kt < C::NST - 2 ? nk - 2 - kt : C::NST - 2;
    pt0 = tick();
    if (kt > 0) pt_work += pt0 - pt1;
    // stage kt+1 was prefetched before the stores for kt + 1 < NST: the stores are younger than it
    if (pre == 2 && COUNTED && kt + 1 < C::NST) mh_wait_stages<NPIECES, COUNTED ? NSTORE : 0>(younger);
    else mh_wait_stages<NPIECES>(younger);
    mh_wait_lgkmcnt0();   // lgkmcnt(0)
    pt1 = tick();
    pt_wait += pt1 - pt0;
    __builtin_amdgcn_s_barrier();
    pt0 = tick();
    pt_bar += pt0 - pt1;
    pt1 = pt0;
    if (kt + C::NST < nk) issue(kt + C::NST);   // slot kt % NST: every wave has read stage kt out of it
    // the W fragments of stage kt + 1 are read straight into b[] behind the LAST MFMA row of this step (their latency falls under the next
    // step's wait + barrier): no second register set, no copy
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      mfma_row(i);
      a[i] = read_frag(As + a_off + i * (16 * 64));
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < TJ; ++j) b[j] = read_frag(Ws + b_offs[j]);
  };
  for (int kt = 0; kt + 1 < nk; ++kt) kstep(kt);
#pragma unroll
  for (int i = 0; i < TI; ++i) mfma_row(i);
  if constexpr ((DBG & 16) != 0) {
    const unsigned long long pc1 = __builtin_amdgcn_s_memtime(), pr1 = __builtin_amdgcn_s_memrealtime();
    if (prof && (threadIdx.x & 63) == 0) {
      prof[0] = (unsigned)pt_wait; prof[1] = (unsigned)pt_bar; prof[2] = (unsigned)pt_work; prof[3] = (unsigned)nk;
      prof[4] = (unsigned)(pc1 - pc0); prof[5] = (unsigned)(pr1 - pr0);
    }
  }
}

// Ping-pong main loop (one block of 8 waves per CU).  The two wave rows (group = wm) run half a K-step
// apart: while one group issues its 32 MFMAs at raised priority, the other - its partner wave on every SIMD -
// reads its 12 fragments of the next K-step from LDS and issues its share of the DMA (an LDS-DMA piece
// costs the ISSUING wave ~100 cycles; put behind the partner's MFMAs it costs the matrix pipe nothing).
// Slots are separated by block-wide raw barriers; group 1 enters one barrier late and group 0 leaves one late.
//   group 0: slot 2kt = LOAD(kt), slot 2kt+1 = MFMA(kt);   group 1: slot 2kt+1 = LOAD(kt), slot 2kt+2 = MFMA(kt)
//   LOAD(kt) reads stage kt and issues stage kt+NST-1 into the ring slot of stage kt-1, whose last readers
//   (group 1, slot 2kt-1) drained lgkmcnt before the barrier that opens slot 2kt;
//   every wave retires its pieces of stage kt+1 at the end of slot 2kt+1, before the barrier that opens the
//   slot in which group 0 reads it - two younger stages stay in flight across that barrier.
template <class C, bool SWAP, int DBG>
__device__ __forceinline__ void pp_mainloop(f32x4 (&acc)[C::TI][C::TJ], const char* smem, const char* const (&srcA)[C::PA],
                                            const char* const (&srcW)[C::PW], const int (&ldsA)[C::PA], const int (&ldsW)[C::PW],
                                            int nk, int a_off, const int (&b_offs)[C::TJ], int64_t kstepA, int64_t kstepW,
                                            int group, bool pre, const BufDma* bd = nullptr) {
  constexpr int TI = C::TI, TJ = C::TJ, D = C::NST - 1;
  static_assert(C::WM == 2, "ping-pong needs exactly two wave rows");
  auto issue = [&](int kt) {
    if constexpr ((DBG & 16384) != 0) issue_stage_buf<C>(smem, *bd, ldsA, ldsW, kt);
    else issue_stage<C, DBG>(smem, srcA, srcW, ldsA, ldsW, kt, kstepA, kstepW);
  };
  auto read_frag = [&](const char* p) -> bf16x8 {
    if constexpr ((DBG & 8) != 0) { bf16x8 v; asm volatile("" : "=v"(v)); return v; }
    else return *reinterpret_cast<const bf16x8*>(p);
  };
  const int npro = nk < D ? nk : D;
  if (pre) {
    mh_wait_vmcnt<0>();
  } else {
    for (int st = 0; st < npro; ++st) issue(st);
    mh_wait_stages<C::PIECES>(npro - 1);
  }
  __builtin_amdgcn_s_barrier();
  if (group == 1) __builtin_amdgcn_s_barrier();
  bf16x8 a[TI], b[TJ];
  for (int kt = 0; kt < nk; ++kt) {
    const char* As = smem + (kt % C::NST) * C::STAGE;
    const char* Ws = As + C::BM * 64;
    const int younger = nk - 2 - kt < D - 1 ? nk - 2 - kt : D - 1;   // stages issued after kt+1 by the end of slot 2kt+1
    // ---- LOAD(kt)
#pragma unroll
    for (int j = 0; j < TJ; ++j) b[j] = read_frag(Ws + b_offs[j]);
#pragma unroll
    for (int i = 0; i < TI; ++i) a[i] = read_frag(As + a_off + i * (16 * 64));
    if (kt + D < nk) issue(kt + D);
    if (group == 1 && kt + 1 < nk) mh_wait_stages<C::PIECES>(younger);
    mh_wait_lgkmcnt0();   // lgkmcnt(0): fragments in registers, ring slot released
    __builtin_amdgcn_s_barrier();
    // ---- MFMA(kt)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      if constexpr ((DBG & 2) != 0) {
        asm volatile("" ::"v"(a[i]));
#pragma unroll
        for (int j = 0; j < TJ; ++j) asm volatile("" ::"v"(b[j]));
      } else {
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          if constexpr (SWAP) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if (group == 0 && kt + 1 < nk) mh_wait_stages<C::PIECES>(younger);
    __builtin_amdgcn_s_barrier();
  }
  if (group == 0) __builtin_amdgcn_s_barrier();
}

template <class C, bool SWAP, int DBG, int NSTORE = 0>
__device__ __forceinline__ void run_mainloop(f32x4 (&acc)[C::TI][C::TJ], const char* smem, const char* const (&srcA)[C::PA],
                                             const char* const (&srcW)[C::PW], const int (&ldsA)[C::PA], const int (&ldsW)[C::PW],
                                             int nk, int a_off, const int (&b_offs)[C::TJ], int64_t kstepA, int64_t kstepW,
                                             int group, int pre, unsigned* prof = nullptr, const BufDma* bd = nullptr) {
  if constexpr (C::PP) pp_mainloop<C, SWAP, DBG>(acc, smem, srcA, srcW, ldsA, ldsW, nk, a_off, b_offs, kstepA, kstepW, group, pre != 0, bd);
  else big_mainloop<C, SWAP, DBG, NSTORE>(acc, smem, srcA, srcW, ldsA, ldsW, nk, a_off, b_offs, kstepA, kstepW, pre, prof, bd);
}

// EPI: 0 generic (bias / act / residual), 1 QKV head scatter, 3 bias + residual + LayerNorm over complete rows
template <class C, int EPI, int ACT, int DBG = 0>
__global__ __launch_bounds__(C::THREADS, C::STAGE * C::NST <= 80 * 1024 ? 2 : 1) void gemm_big_kernel(const GemmArgs g) {
  // LDS: the DMA ring, then (EPI 3) the row-statistics exchange - kept apart so that the next tile's first
  // stages can already be landing in the ring while this tile's epilogue runs
  // (EPI 3 also keeps bias / LayerNorm gain / shift of the block's BN = N columns in LDS: read back with ds_read in the epilogue,
  // they cost neither vector registers across the main loop nor vmcnt waits between the stores)
  // deferred LayerNorm (DeferArgs), one compiled variant per operand combination so that unused vectors cost no registers:
  // DA = A rows raw, DR = residual rows raw, DO = write the output rows' partial statistics
  constexpr bool DA = (DBG & 128) != 0, DR = (DBG & 256) != 0, DO = (DBG & 512) != 0, DEFER = DA || DR || DO;
  constexpr int TI_ = C::TI, TJ_ = C::TJ;
  // (EPI 3 stages the tile's residual rows through LDS after the main loop: each wave's TI x TJ/2 KiB go where the ring was;
  // a last wave that does not fit - the 128x512 tile: 8 x 16 KiB against a 120 KiB ring - gets its own area at the end)
  constexpr int RES_W = TI_ * (TJ_ / 2) * 1024, RING = C::NST * C::STAGE;
  constexpr bool RES_EXTRA = EPI == 3 && C::NW * RES_W > RING;
  static_assert(EPI != 3 || (C::NW - 1) * RES_W <= RING, "residual staging: at most the last wave may overflow the ring");
  // EPI 0, DBG bits 16..19 (round 6): the FORM of the epilogue fixed at compile time - 1 plain (no residual), 2 residual add, 4 the residual
  // tensor holds act'(pre) and multiplies (the backward's act-grad GEMM), 8 ACT = GELU with gelu'(pre) as a second output (the training
  // forward's FFN1); 0 = generic: `residual`, `act_grad`, `out_f32`, `pre_out` are looked at per 8-value group.  They are wave-uniform and
  // loop-invariant, but hipcc unswitches them into 20 - 27 thousand instructions per kernel (the straight-line forms have 4 - 5 thousand: the
  // difference is the instruction cache); launch_big picks the form
  constexpr int FORM = (DBG >> 16) & 15;
  constexpr bool GEN = FORM == 0;
  static_assert(GEN || (EPI == 0 && !DEFER && (DBG & 64) == 0 && (FORM == 1 || FORM == 2 || FORM == 4 || (FORM == 8 && ACT == MH_ACT_GELU_ERF))), "fixed epilogue forms: EPI 0, no deferred LayerNorm, no dropout");
  __shared__ __attribute__((aligned(16))) char smem[C::NST * C::STAGE + (EPI == 3 ? C::BM * C::WN * 4 + 3 * C::BN * 4 : 0) +
                                                    (DEFER ? C::BM * 8 * (2 + C::WN) : 0) + (RES_EXTRA ? RES_W : 0)];
  constexpr int TI = C::TI, TJ = C::TJ;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / C::WN, wn = wave % C::WN;
  const int tiles_n = (g.N + C::BN - 1) / C::BN;
  const int nk = g.K / B2K;
  const int fr = lane & 15, fg = lane >> 4;
  // DMA coordinates: one piece covers 16 rows x 64 B; lane i lands at row i/4, physical chunk i%4.
  // row-major operand: rows ld elements apart, a K-step advances 32 elements; K32-panel operand
  // ([K/32][ld rows][32]): rows 32 elements apart, a K-step advances one whole panel (ld * 32)
  const char* srcA[C::PA];
  const char* srcW[C::PW];
  int ldsA[C::PA], ldsW[C::PW];
  const int64_t a_row = g.a_panel ? 32 : g.lda, w_row = g.w_panel ? 32 : g.ldw;
  const int64_t kstepA = g.a_panel ? g.lda * 64 : 64, kstepW = g.w_panel ? g.ldw * 64 : 64;
#pragma unroll
  for (int j = 0; j < C::PA; ++j) ldsA[j] = ((wave * C::PA + j) % C::APIECES) * 16 * 64;
#pragma unroll
  for (int j = 0; j < C::PW; ++j) ldsW[j] = (wave * C::PW + j) * 16 * 64;
  constexpr bool BUFDMA = (DBG & 16384) != 0;
  static_assert(!BUFDMA || ((C::APIECES % C::NW == 0 || C::PA == 1) && C::PA * 1024 <= 4096 && C::PW * 1024 <= 4096),
                "buffer DMA: a wave's pieces of a stage must be consecutive (immediate offsets of 1 KiB, 12 bits)");
  BufDma bd;
  if constexpr (BUFDMA) {
    const int rl = lane >> 2, lc = (lane & 3) ^ MH_GSW[(rl >> 2) & 3];
    bd.va = (((wave * C::PA) % C::APIECES) * 16 + rl) * 64 + lc * 16;
    bd.vw = ((wave * C::PW) * 16 + rl) * 64 + lc * 16;
    bd.ka = (int)(g.lda * 64);
    bd.kw = (int)(g.ldw * 64);
  }
  auto set_sources = [&](int tile) {
    const int b2 = mh_xcd_remap(tile, g.ntiles);
    const int64_t tm0 = (int64_t)(b2 / tiles_n) * C::BM;
    const int tn0 = (b2 % tiles_n) * C::BN;
    if constexpr (BUFDMA) {   // (panel operands: row r of panel 0 at byte 64 r; everything here is wave-uniform)
      const int64_t offA = ((int64_t)blockIdx.y * g.sA) * 2 + tm0 * 64, offW = ((int64_t)blockIdx.y * g.sW) * 2 + (int64_t)tn0 * 64;
      // the bound of mh_panel_rsrc (lds_dma.h: the rows this operand OWNS in its last panel), spelled out here: see the note there
      const int64_t bytesA = (int64_t)(g.K / 32 - 1) * g.lda * 64 + (g.M - tm0) * 64, bytesW = (int64_t)(g.K / 32 - 1) * g.ldw * 64 + ((int64_t)g.N - tn0) * 64;
      bd.ra = mh_buf_rsrc(reinterpret_cast<const char*>(g.A) + offA, (int)bytesA);
      bd.rw = mh_buf_rsrc(reinterpret_cast<const char*>(g.W) + offW, (int)bytesW);
      return;
    }
    const int rl = lane >> 2, pc = lane & 3;
    const int lc = pc ^ MH_GSW[(rl >> 2) & 3];          // logical chunk stored at this physical slot
#pragma unroll
    for (int j = 0; j < C::PA; ++j) {
      int64_t ra = tm0 + ((wave * C::PA + j) % C::APIECES) * 16 + rl; if (ra >= g.M) ra = g.M - 1;
      srcA[j] = reinterpret_cast<const char*>(g.A) + ((int64_t)blockIdx.y * g.sA + ra * a_row + lc * 8) * 2;
    }
#pragma unroll
    for (int j = 0; j < C::PW; ++j) {
      int rw = tn0 + (wave * C::PW + j) * 16 + rl; if (rw >= g.N) rw = g.N - 1;
      srcW[j] = reinterpret_cast<const char*>(g.W) + ((int64_t)blockIdx.y * g.sW + (int64_t)rw * w_row + lc * 8) * 2;
    }
  };
  if constexpr (EPI == 3) {
    float* vecs = reinterpret_cast<float*>(smem + C::NST * C::STAGE + C::BM * C::WN * 4);
    for (int c = tid; c < C::BN; c += C::THREADS) {
      vecs[c] = g.bias[c];
      vecs[C::BN + c] = g.ln_gamma[c];
      vecs[2 * C::BN + c] = g.ln_beta[c];
    }
    __syncthreads();
  }
  int pre = 0;   // 1 / 2: this tile's first stages were issued before the previous tile's epilogue (2: a full tile's, see big_mainloop)
  // persistent: after a tile's main loop the ring is idle, so the next tile's first stages are put in flight
  // BEFORE the epilogue: their latency (an HBM miss for the A rows) hides behind the stores
  auto prefetch_next = [&](int vt, bool full_tile) {
    const int vn = vt + (int)gridDim.x;
    pre = 0;
    if constexpr (EPI == 3) return;   // the row-statistics epilogue has no registers to spare for the carried pointers
    if constexpr (DEFER) return;      // (its epilogue holds the row statistics: no registers to spare either)
    if (g.dbg & 32) return;           // A/B: no prefetch across the epilogue
    if (vn < g.ntiles) {
      set_sources(vn);
      if constexpr (!C::PP) {   // (the ping-pong loop ends on a barrier that every fragment read precedes)
        mh_wait_lgkmcnt0();
        __builtin_amdgcn_s_barrier();
      }
      const int npro = nk < C::PRO ? nk : C::PRO;
      for (int st = 0; st < npro; ++st) {
        if constexpr (BUFDMA) issue_stage_buf<C>(smem, bd, ldsA, ldsW, st);
        else issue_stage<C, DBG>(smem, srcA, srcW, ldsA, ldsW, st, kstepA, kstepW);
      }
      pre = (full_tile && nk >= C::NST && !(g.dbg & 64)) ? 2 : 1;   // (dbg bit 64: A/B, always drain)
    }
  };
  // DEFER: (mean, rstd) of the tile's A rows / residual rows from the producers' partial sums, staged in LDS for every wave
  float2* lds_a = reinterpret_cast<float2*>(smem + C::NST * C::STAGE);
  float2* lds_r = lds_a + C::BM;
  float2* lds_o = lds_r + C::BM;      // [BM][WN]
  auto stage_row_stats = [&](int64_t m0) {
    if constexpr (DA || DR) {
      for (int t = tid; t < C::BM; t += C::THREADS) {
        int64_t row = m0 + t; if (row >= g.M) row = g.M - 1;
        if constexpr (DA) {
          float s1 = 0.f, s2 = 0.f;
          for (int sl = 0; sl < g.d.a_slots; ++sl) { const float2 p = reinterpret_cast<const float2*>(g.d.a_stats)[row * g.d.a_slots + sl]; s1 += p.x; s2 += p.y; }
          const float mean = s1 * g.d.inv_h, var = fmaxf(s2 * g.d.inv_h - mean * mean, 0.f);
          lds_a[t] = float2{mean, 1.0f / sqrtf(var + g.d.eps)};
        }
        if constexpr (DR) {
          float s1 = 0.f, s2 = 0.f;
          for (int sl = 0; sl < g.d.r_slots; ++sl) { const float2 p = reinterpret_cast<const float2*>(g.d.r_stats)[row * g.d.r_slots + sl]; s1 += p.x; s2 += p.y; }
          const float mean = s1 * g.d.inv_h, var = fmaxf(s2 * g.d.inv_h - mean * mean, 0.f);
          lds_r[t] = float2{mean, 1.0f / sqrtf(var + g.d.eps)};
        }
      }
      mh_wait_lgkmcnt0_fence();
      __builtin_amdgcn_s_barrier();
    }
  };
  for (int vt = blockIdx.x; vt < g.ntiles; vt += gridDim.x) {
  if (!pre) {
    if (vt != (int)blockIdx.x) {   // the ring is reused: every wave must be done reading the previous tile's last stage
      mh_wait_lgkmcnt0();
      __builtin_amdgcn_s_barrier();
    }
    set_sources(vt);
  }
  const int bid = mh_xcd_remap(vt, g.ntiles);
  const int64_t m0 = (int64_t)(bid / tiles_n) * C::BM;
  const int n0 = (bid % tiles_n) * C::BN;
  const int frag_off = fr * 64 + ((fg ^ MH_GSW[(fr >> 2) & 3]) << 4);
  const int a_off = wm * (TI * 16 * 64) + frag_off;
  const int wcol0 = n0 + wn * (TJ * 16);
  const int64_t wrow0 = m0 + wm * (TI * 16);
  const bool v_wave = (EPI == 1) && (wcol0 / g.H == 2);
  const bool full_tile = m0 + C::BM <= g.M && n0 + C::BN <= g.N;   // every lane stores every element: the store count per wave is known
  int b_offs[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int jj = j & 3;
    const int row = (j >> 2) * 64 + (v_wave ? 16 * jj + fr : 32 * (jj >> 1) + 8 * (fr >> 2) + 4 * (jj & 1) + (fr & 3));
    b_offs[j] = wn * (TJ * 16 * 64) + row * 64 + ((fg ^ MH_GSW[(row >> 2) & 3]) << 4);
  }

  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (DA || DR) {
    // deferred LayerNorm: the tile's first DMA stages go out first and the row statistics (a global round trip + a barrier) are
    // fetched underneath them, instead of standing between the main loop and the epilogue
    if (!pre) {
      const int npro = nk < C::PRO ? nk : C::PRO;
      for (int st = 0; st < npro; ++st) {
        if constexpr (BUFDMA) issue_stage_buf<C>(smem, bd, ldsA, ldsW, st);
        else issue_stage<C, DBG>(smem, srcA, srcW, ldsA, ldsW, st, kstepA, kstepW);
      }
      pre = 1;
    }
    stage_row_stats(m0);
  }
  // lane's 8 consecutive output columns for (64-column group q, half h): wcol0 + 64q + 32h + 8fg, values
  // acc[i][4q + 2h + (e>>2)][e&3], e = 0..7
  if constexpr (EPI == 1) {
    const int which = wcol0 / g.H;   // wave-uniform: 0 q, 1 k, 2 v
    const int M32 = (int)g.M, r0 = (int)wrow0;
    if (which == 2) {
      run_mainloop<C, false, DBG, TI * TJ>(acc, smem, srcA, srcW, ldsA, ldsW, nk, a_off, b_offs, kstepA, kstepW, wm, pre, nullptr, &bd);
      prefetch_next(vt, full_tile);
      // acc[i][j][r] = D[m = 16i + 4fg + r][n = 16j + fr]: 4 consecutive tokens per lane -> V^T rows
      // FULL (interior tile, wave-uniform): no per-lane guards, so the epilogue is straight-line code.  With divergent guards
      // hipcc cannot prove the bias loads complete on every path and puts `s_waitcnt vmcnt(0)` in front of EVERY store block,
      // which also waits for the previous store: the tile's stores then leave one round trip at a time.
      auto epi_v = [&](auto fullc) {
        constexpr bool FULL = decltype(fullc)::value;
        bf16* dst = reinterpret_cast<bf16*>(g.vt);
        float bv[TJ], c1v[TJ];
        int64_t coloff[TJ];
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int col = wcol0 + 16 * j + fr;
          const int cc = (FULL || col < g.N) ? col : g.N - 1;
          bv[j] = g.bias[cc];
          if constexpr (DA) c1v[j] = g.d.c1[cc];
          const int c = cc - 2 * g.H, head = c / g.dh, d = c % g.dh;
          coloff[j] = (FULL || col < g.N) ? ((int64_t)head * g.dh + d) * g.L : -1;
        }
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const int row = r0 + 16 * i + 4 * fg;
          if (FULL || row < M32) {
            const int b = row / g.L;
            int l = row - b * g.L;
            if (g.vt_perm) l = (l & ~15) | ((((l >> 3) & 1) | ((l >> 1) & 2)) << 2);   // 4-token group 0,1,2,3 -> 0,2,1,3
            bf16* base = dst + (int64_t)b * g.H * g.L + l;
            float mu[4] = {0.f, 0.f, 0.f, 0.f}, rsd[4] = {1.f, 1.f, 1.f, 1.f};
            if constexpr (DA) {   // rows 16 i + 4 fg + r of the tile: four consecutive (mean, rstd) pairs
              const f32x4* sp = reinterpret_cast<const f32x4*>(lds_a + wm * (TI * 16) + 16 * i + 4 * fg);
              const f32x4 s01 = sp[0], s23 = sp[1];
              mu[0] = s01[0]; rsd[0] = s01[1]; mu[1] = s01[2]; rsd[1] = s01[3];
              mu[2] = s23[0]; rsd[2] = s23[1]; mu[3] = s23[2]; rsd[3] = s23[3];
            }
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
              if (FULL || coloff[j] >= 0) {
                bf16x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  if constexpr (DA) v[r] = (bf16)fmaf(rsd[r], fmaf(-mu[r], c1v[j], acc[i][j][r]), bv[j]);
                  else v[r] = (bf16)(acc[i][j][r] + bv[j]);
                }
                *reinterpret_cast<bf16x4*>(base + coloff[j]) = v;
              }
            }
          }
        }
      };
      if (full_tile) epi_v(std::true_type{}); else epi_v(std::false_type{});
    } else {
      run_mainloop<C, true, DBG, TI * (TJ / 2)>(acc, smem, srcA, srcW, ldsA, ldsW, nk, a_off, b_offs, kstepA, kstepW, wm, pre, nullptr, &bd);
      prefetch_next(vt, full_tile);
      auto epi_qk = [&](auto fullc) {
        constexpr bool FULL = decltype(fullc)::value;
        bf16* dst = reinterpret_cast<bf16*>(which == 0 ? g.q : g.k);
        float bv[TJ / 2][8];          // every bias load before the first store: a load behind a store would wait for it
        float c1v[TJ / 2][8];
        float mu[TI], rsd[TI];
        const bool scale_q = which == 0 && g.q_scale != 0.f;   // (wave-uniform)
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
          load8(g.bias + ((FULL || col < g.N) ? col : 0), bv[qh]);
          if constexpr (DA) load8(g.d.c1 + ((FULL || col < g.N) ? col : 0), c1v[qh]);
        }
        if constexpr (DA) {
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            const float2 st = lds_a[wm * (TI * 16) + 16 * i + fr];
            mu[i] = st.x; rsd[i] = st.y;
          }
        }
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
          if (FULL || col < g.N) {
            const int c = col - which * g.H, head = c / g.dh, d = c % g.dh;
            const int64_t coloff = (int64_t)head * g.L * g.dh + d;
#pragma unroll
            for (int i = 0; i < TI; ++i) {
              const int row = r0 + 16 * i + fr;
              if (FULL || row < M32) {
                const int b = row / g.L, l = row - b * g.L;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  if constexpr (DA) v[e] = fmaf(rsd[i], fmaf(-mu[i], c1v[qh][e], acc[i][2 * qh + (e >> 2)][e & 3]), bv[qh][e]);
                  else v[e] = acc[i][2 * qh + (e >> 2)][e & 3] + bv[qh][e];
                }
                if (scale_q) {
#pragma unroll
                  for (int e = 0; e < 8; ++e) v[e] *= g.q_scale;
                }
                if constexpr ((DBG & 32) != 0) store8(dst + ((int64_t)b * g.nh * g.L + l) * g.dh + coloff, v);
                else store8_nt(dst + ((int64_t)b * g.nh * g.L + l) * g.dh + coloff, v);
              }
            }
          }
        }
      };
      if (full_tile) epi_qk(std::true_type{}); else epi_qk(std::false_type{});
    }
  } else {
    // stores per wave of a full tile: one 16-byte store per (row tile, 32-column half); a second one with pre_out
    run_mainloop<C, true, DBG, TI * (TJ / 2)>(acc, smem, srcA, srcW, ldsA, ldsW, nk, a_off, b_offs, kstepA, kstepW, wm, pre,
                                              reinterpret_cast<unsigned*>(g.out) + 64 + ((int64_t)bid * C::NW + wave) * 8, &bd);
    prefetch_next(vt, full_tile && !g.pre_out && !g.out_f32);
    bf16* outT = reinterpret_cast<bf16*>(g.out) + (int64_t)blockIdx.y * g.sO;
    float* outF = reinterpret_cast<float*>(g.out) + (int64_t)blockIdx.y * g.sO;
    const bf16* res = g.residual ? reinterpret_cast<const bf16*>(g.residual) + (int64_t)blockIdx.y * g.sR : nullptr;
    if constexpr ((DBG & 4) != 0) {
      float sacc = 0.f;
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) sacc += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
      if (sacc == 12345.678f) outF[0] = sacc;
      continue;
    }
    if constexpr (EPI == 3) {
      // ---- bias + residual, then LayerNorm over the complete row (the block owns all N columns): two-pass
      // statistics, in-lane -> across the 4 lanes of a row (xor 16, 32) -> across the WN waves through LDS.
      // Every global load of the epilogue (the residual rows) is consumed before the first store, and bias / gain / shift come
      // from LDS: with a global load pending behind divergent row guards hipcc puts `s_waitcnt vmcnt(0)` in front of every
      // store, which also waits for the previous store - the tile's stores then leave one round trip at a time.
      {
        constexpr bool FULL = false;
        float* red = reinterpret_cast<float*>(smem + C::NST * C::STAGE);   // [BM][WN] floats, reused for both passes
        const float* vecs = red + C::BM * C::WN;                            // bias | gamma | beta of the BN columns
        // The residual rows take ONE memory round trip: every wave DMAs its own TI x TJ/2 pieces (lane-linear: a lane's 16 bytes of
        // piece (qh, i) are exactly the 8 columns it holds of row 16 i + fr) into the ring the main loop has just left - all waves
        // are past its last barrier - adds the bias while they fly, and reads them back with ds_read_b128 (no other wave touches them).
        // (Loading them group by group into registers cost four dependent round trips: there are no registers for more at once.)
        char* rbase = smem + ((wave + 1) * RES_W <= RING ? wave * RES_W : RING + C::BM * C::WN * 4 + 3 * C::BN * 4);
        if constexpr (!C::PP) {   // (the ping-pong loop ends on a barrier that every fragment read precedes; the plain loop does not)
          mh_wait_lgkmcnt0();
          __builtin_amdgcn_s_barrier();
        }
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            int64_t row = wrow0 + 16 * i + fr; if (!FULL && row >= g.M) row = g.M - 1;
            const int64_t ro = g.r_panel ? ((int64_t)(col >> 5) * g.ldr + row) * 32 + (col & 31) : row * g.ldr + col;
            mh_glds16<MH_EPI3_RES_NT ? 2 : 0>(res + ro, rbase + (qh * TI + i) * 1024);
          }
        }
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          float bv[8];
          load8(vecs + wcol0 + 32 * qh + 8 * fg, bv);
#pragma unroll
          for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[i][2 * qh + (e >> 2)][e & 3] += bv[e];
        }
        if constexpr ((DBG & 64) != 0) {   // train-mode dropout of the dense output, before the residual (same element numbering as EPI 0)
          if (g.drop.thr)                    // (the training build also serves p = 0: it is the one that writes pre_out)
#pragma unroll
          for (int qh = 0; qh < TJ / 2; ++qh) {
            const int col = wcol0 + 32 * qh + 8 * fg;
#pragma unroll
            for (int i = 0; i < TI; ++i) {
              int64_t row = wrow0 + 16 * i + fr; if (row >= g.M) row = g.M - 1;
              const uint32_t km = drop_keep8_at(g.drop, (uint64_t)row * g.N + col);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float a = acc[i][2 * qh + (e >> 2)][e & 3];
                acc[i][2 * qh + (e >> 2)][e & 3] = (km >> e) & 1u ? a * g.drop.rscale : 0.f;
              }
            }
          }
        }
        mh_wait_vmcnt<0>();
        float rs[TI];
#pragma unroll
        for (int i = 0; i < TI; ++i) rs[i] = 0.f;
        // pre_out (training): the un-normalised rows are kept for the LayerNorm backward, rounded to bf16, and the statistics are taken
        // from the ROUNDED values - what a separate LayerNorm kernel reading that tensor would see
        bf16* preT = (DBG & 64) != 0 ? reinterpret_cast<bf16*>(g.pre_out) : nullptr;   // (compile-time off in the sampling build)
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            const bf16x8 rraw = *reinterpret_cast<const bf16x8*>(rbase + (qh * TI + i) * 1024 + lane * 16);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = acc[i][2 * qh + (e >> 2)][e & 3] + (float)rraw[e];
            if (preT) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = (float)(bf16)v[e];
              const int64_t row = wrow0 + 16 * i + fr;
              const int64_t ldp = g.ldp ? g.ldp : g.ldo;
              if (row < g.M) store8_nt(preT + (g.p_panel ? ((int64_t)(col >> 5) * ldp + row) * 32 + (col & 31) : row * ldp + col), v);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              acc[i][2 * qh + (e >> 2)][e & 3] = v[e];
              rs[i] += v[e];
            }
          }
        }
        const float invN = 1.0f / (float)g.N;
        float mean[TI], rstd[TI];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            float v = rs[i];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (fg == 0) red[(wm * (TI * 16) + 16 * i + fr) * C::WN + wn] = v;
          }
          mh_wait_lgkmcnt0_fence();
          __builtin_amdgcn_s_barrier();
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < C::WN; ++w) t += red[(wm * (TI * 16) + 16 * i + fr) * C::WN + w];
            if (pass == 0) {
              mean[i] = t * invN;
              float sq = 0.f;
#pragma unroll
              for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float d = acc[i][j][r] - mean[i]; sq += d * d; }
              rs[i] = sq;
            } else {
              rstd[i] = 1.0f / sqrtf(t * invN + g.ln_eps);
            }
          }
          __builtin_amdgcn_s_barrier();                    // reads done before the second pass overwrites `red`
        }
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
          float gv[8], bt[8];
          load8(vecs + C::BN + col, gv);
          load8(vecs + 2 * C::BN + col, bt);
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            const int64_t row = wrow0 + 16 * i + fr;
            if (FULL || row < g.M) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = (acc[i][2 * qh + (e >> 2)][e & 3] - mean[i]) * rstd[i] * gv[e] + bt[e];
              const int64_t oo = g.o_panel ? ((int64_t)(col >> 5) * g.ldo + row) * 32 + (col & 31) : row * g.ldo + col;
              store8(outT + oo, v);   // ordinary store: the next GEMM re-reads these rows (A operand and residual) from L2 / MALL
            }
          }
        }
      }
    } else {
      auto epi_gen = [&](auto fullc) {
        constexpr bool FULL = decltype(fullc)::value;
        float bv[TJ / 2][8];          // every bias load before the first store
        // element offsets as (column part) + (row part), the row part advanced by additions: a 64-bit multiply per store is three
        // quarter-rate instructions, and the epilogue is vector-bound
        const int64_t o_rs = g.o_panel ? 32 : g.ldo, r_rs = g.r_panel ? 32 : g.ldr;     // elements between consecutive rows
        const int64_t o_row0 = (wrow0 + fr) * o_rs, r_row0 = (wrow0 + fr) * r_rs;
        float os1[TI], os2[TI];       // DO: running (sum, sum of squares) of this lane's part of each row
        if constexpr (DO) {
#pragma unroll
          for (int i = 0; i < TI; ++i) { os1[i] = 0.f; os2[i] = 0.f; }
        }
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
#pragma unroll
          for (int e = 0; e < 8; ++e) bv[qh][e] = 0.f;
          if (g.bias && (FULL || col < g.N)) {
            if (FULL || col + 8 <= g.N) load8(g.bias + col, bv[qh]);
            else { const f32x4 b4 = *reinterpret_cast<const f32x4*>(g.bias + col); bv[qh][0] = b4[0]; bv[qh][1] = b4[1]; bv[qh][2] = b4[2]; bv[qh][3] = b4[3]; }
          }
        }
        // DR (round 6): the tile's residual rows take ONE round trip through the idle ring (LDS-DMA, lane-linear pieces: a lane's 16 bytes of
        // piece (qh, i) are the 8 columns it holds of row 16 i + fr - the EPI 3 epilogue's scheme) instead of TI x 4 registers per column
        // group: with them the raw-residual + output-statistics kernel (the attention-output and FFN-output dense of every d_model 768 layer)
        // needed 287 registers, spilled 31, and ran 40.2 us where either feature alone runs 29.3 - 30.6 (tools/debug/defer_epilogue_bench.py)
        constexpr bool RSTAGE = DR && !C::PP && C::NW * (TI * (TJ / 2) * 1024) <= C::NST * C::STAGE;
        const char* rstage = smem + wave * (TI * (TJ / 2) * 1024);
        const char* gbstage = smem + C::NW * (TI * (TJ / 2) * 1024) + wave * 1024;
        if constexpr (RSTAGE) {
          mh_wait_lgkmcnt0();      // (the plain main loop does not end on a barrier: every wave's fragment reads first)
          __builtin_amdgcn_s_barrier();
#pragma unroll
          for (int qh = 0; qh < TJ / 2; ++qh) {
            const int col = wcol0 + 32 * qh + 8 * fg;
            const int cc = (FULL || col + 8 <= g.N) ? col : 0;
            const int64_t r_col = g.r_panel ? (int64_t)(cc >> 5) * g.ldr * 32 + (cc & 31) : cc;
#pragma unroll
            for (int i = 0; i < TI; ++i) {
              int64_t row = wrow0 + 16 * i + fr; if (!FULL && row >= g.M) row = g.M - 1;
              mh_glds16(res + r_col + row * r_rs, const_cast<char*>(rstage + (qh * TI + i) * 1024));
            }
          }
          // ... and the wave's 64 residual gains | shifts ride along as one more piece (lanes 0 - 15 gamma, 16 - 31 beta, the rest repeat):
          // read back per row tile, they are not live across the column group's rows (16 registers fewer)
          static_assert(!RSTAGE || C::NW * (TI * (TJ / 2) * 1024) + C::NW * 1024 <= C::NST * C::STAGE, "no room for the gain / shift pieces");
          {
            const int l32 = lane & 31, gc = wcol0 + 4 * (l32 & 15);
            const float* gsrc = (l32 < 16 ? g.d.r_gamma : g.d.r_beta) + ((FULL || gc + 4 <= g.N) ? gc : 0);
            mh_glds16(gsrc, const_cast<char*>(gbstage));
          }
          mh_wait_vmcnt<0>();     // (the bias loads above included: nothing the epilogue loads is pending behind its first store)
        }
#pragma unroll
        for (int qh = 0; qh < TJ / 2; ++qh) {
          const int col = wcol0 + 32 * qh + 8 * fg;
          if (FULL || col < g.N) {   // N % 8 == 0, or an fp32 output with N % 8 == 4 (big_tile_ok): at least the first 4 columns are valid
            float c1v[8], rgv[8], rbv[8];   // deferred-LayerNorm column vectors of this group (loaded with its residual rows)
            if constexpr (DA) load8(g.d.c1 + ((FULL || col + 8 <= g.N) ? col : 0), c1v);
            if constexpr (DR && !RSTAGE) { load8(g.d.r_gamma + ((FULL || col + 8 <= g.N) ? col : 0), rgv); load8(g.d.r_beta + ((FULL || col + 8 <= g.N) ? col : 0), rbv); }
            bf16x8 rraw[RSTAGE ? 1 : TI];         // the group's residual rows: all loads in flight together, behind the previous group's stores
            if constexpr (!RSTAGE) if (GEN ? res != nullptr : (FORM & 6) != 0) {
              const int64_t r_col = g.r_panel ? (int64_t)(col >> 5) * g.ldr * 32 + (col & 31) : col;
              int64_t ro = r_col + r_row0;
#pragma unroll
              for (int i = 0; i < TI; ++i) {
                if (FULL || wrow0 + 16 * i + fr < g.M) rraw[i] = *reinterpret_cast<const bf16x8*>(res + ro);
                else rraw[i] = *reinterpret_cast<const bf16x8*>(res + r_col + (g.M - 1) * r_rs);
                ro += 16 * r_rs;
              }
            }
            const int64_t o_col = g.o_panel ? (int64_t)(col >> 5) * g.ldo * 32 + (col & 31) : col;
            int64_t oo = o_col + o_row0 - 16 * o_rs;
#pragma unroll
            for (int i = 0; i < TI; ++i) {
              const int64_t row = wrow0 + 16 * i + fr;
              oo += 16 * o_rs;
              if (FULL || row < g.M) {
                float v[8];
                const int rt = wm * (TI * 16) + 16 * i + fr;     // row of the tile: (mean, rstd) pairs staged in LDS
                if constexpr (DA) {
                  const float2 sa = lds_a[rt];
#pragma unroll
                  for (int e = 0; e < 8; ++e) v[e] = fmaf(sa.y, fmaf(-sa.x, c1v[e], acc[i][2 * qh + (e >> 2)][e & 3]), bv[qh][e]);
                } else {
#pragma unroll
                  for (int e = 0; e < 8; ++e) v[e] = acc[i][2 * qh + (e >> 2)][e & 3] + bv[qh][e];
                }
                if constexpr (ACT != MH_ACT_NONE) {
                  bool done = false;
                  if constexpr (ACT == MH_ACT_GELU_ERF) {
                    if (FORM == 8 || (GEN && !DEFER && g.pre_out && g.pre_kind == 1)) {   // training: the backward gets gelu'(pre), from the same exp / rcp as gelu(pre)
                      float gp[8];
                      gelu_erf_fast8_dgelu(v, gp);
                      store8_nt(reinterpret_cast<bf16*>(g.pre_out) + (int64_t)blockIdx.y * g.sO + oo, gp);
                      done = true;
                    }
                  }
                  if (!done) {
                    if (GEN && !DEFER && g.pre_out) {   // training: the backward needs the pre-activation
                      store8_nt(reinterpret_cast<bf16*>(g.pre_out) + (int64_t)blockIdx.y * g.sO + oo, v);
                    }
                    if constexpr (ACT == MH_ACT_GELU_ERF) gelu_erf_fast8(v);
                    else {
#pragma unroll
                      for (int e = 0; e < 8; ++e) v[e] = apply_act<bf16>(v[e], ACT);
                    }
                  }
                }
                if constexpr ((DBG & 64) != 0) {   // train-mode dropout of the dense output, before the residual
                  const uint32_t km = drop_keep8_at(g.drop, (uint64_t)row * g.N + col);
#pragma unroll
                  for (int e = 0; e < 8; ++e) v[e] = (km >> e) & 1u ? v[e] * g.drop.rscale : 0.f;
                }
                // (the deferred-LayerNorm kernels - launch_big sees to it - have no activation gradient, no fp32 output, and with DR always a
                // residual: compile-time there, so that a group is straight-line code instead of a dozen uniform branches)
                if (DR || (GEN ? res != nullptr : (FORM & 6) != 0)) {
                  bf16x8 rv;
                  if constexpr (RSTAGE) rv = *reinterpret_cast<const bf16x8*>(rstage + (qh * TI + i) * 1024 + lane * 16);
                  else rv = rraw[RSTAGE ? 0 : i];
                  if (GEN && !DEFER && g.act_grad == MH_ACT_GELU_ERF) {          // backward of dense + GELU: dpre = (dY W) o gelu'(pre)
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= gelu_erf_grad((float)rv[e]);
                  } else if (FORM == 4 || (GEN && !DEFER && g.act_grad == MH_ACT_DERIV)) {        // the tensor holds act'(pre) already (mh_gemm_bias_act_dact)
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= (float)rv[e];
                  } else if (GEN && !DEFER && g.act_grad == MH_ACT_TANH) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float th = tanhf((float)rv[e]); v[e] *= 1.0f - th * th; }
                  } else if constexpr (DR) {
                    const float2 sr = lds_r[rt];
                    if constexpr (RSTAGE) {
                      load8(reinterpret_cast<const float*>(gbstage) + 32 * qh + 8 * fg, rgv);
                      load8(reinterpret_cast<const float*>(gbstage + 256) + 32 * qh + 8 * fg, rbv);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += fmaf(((float)rv[e] - sr.x) * sr.y, rgv[e], rbv[e]);
                  } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += (float)rv[e];
                  }
                }
                if constexpr (DO) {   // statistics of the row as the consumers will read it: from the bf16-rounded values
#pragma unroll
                  for (int e = 0; e < 8; ++e) { const float r = (float)(bf16)v[e]; os1[i] += r; os2[i] += r * r; }
                }
                if (GEN && !DEFER && g.out_f32) {
                  if (FULL || col + 8 <= g.N) store8(outF + oo, v);
                  else *reinterpret_cast<f32x4*>(outF + oo) = f32x4{v[0], v[1], v[2], v[3]};   // N % 8 == 4 tail
                } else {
                  // streaming stores for outputs read once, much later or by a streaming reader; the deferred-LayerNorm producers' raw
                  // rows are re-read at once as A operand and residual: ordinary stores (c2-bertbase -2.0 % step time, A/B of two builds)
                  if constexpr ((DBG & 2048) != 0) {   // timing-only ablation: the epilogue's arithmetic without its stores (values kept live)
                    float keep = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) keep += v[e];
                    if (keep == 12345.678f) store8(outT + oo, v);
                  }
                  else if constexpr ((DBG & 32) != 0 || DO) store8(outT + oo, v); else store8_nt(outT + oo, v);
                }
              }
            }
          }
        }
        if constexpr (DO) {
          {   // fold the lane partials over the 4 lanes of a row, then over the WN column waves (fixed order)
#pragma unroll
            for (int i = 0; i < TI; ++i) {
              float a = os1[i], b = os2[i];
              a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
              b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
              if (fg == 0) lds_o[(wm * (TI * 16) + 16 * i + fr) * C::WN + wn] = float2{a, b};
            }
            mh_wait_lgkmcnt0_fence();
            __builtin_amdgcn_s_barrier();
            for (int t = tid; t < C::BM; t += C::THREADS) {
              float a = 0.f, b = 0.f;
#pragma unroll
              for (int w = 0; w < C::WN; ++w) { const float2 p = lds_o[t * C::WN + w]; a += p.x; b += p.y; }
              if (m0 + t < g.M) reinterpret_cast<float2*>(g.d.o_stats)[(m0 + t) * g.d.o_slots + n0 / C::BN] = float2{a, b};
            }
          }
        }
      };
      if (full_tile) epi_gen(std::true_type{}); else epi_gen(std::false_type{});
    }
  }
  }   // persistent tile loop
}

}  // namespace

template <class C, int EPI>
int launch_big(const GemmArgs& g0, hipStream_t s, int batch) {
  GemmArgs g = g0;
  const int64_t t2 = (int64_t)ceil_div(g.M, C::BM) * ceil_div(g.N, C::BN);
  MH_CHECK_ARG(t2 > 0 && t2 < (1ll << 31), "gemm: bad grid (M=%lld N=%d)", (long long)g.M, g.N);
  // persistent: one block per CU slot walks the tiles (no re-launch, the ring stays allocated)
  const int cus = mh_device_cus();
  const int per_cu = (C::STAGE * C::NST <= 80 * 1024 && C::NW <= 4) ? 2 : 1;
  const int64_t slots = (int64_t)cus * per_cu;
  g.ntiles = (int)t2;
  const dim3 grid((unsigned)(t2 < slots ? t2 : slots), (unsigned)batch), block(C::THREADS);
  mh_prof_note("tile=%dx%d%s epi=%d act=%d M=%lld N=%d K=%d batch=%d", C::BM, C::BN, C::PP ? "pp" : "", EPI, g.act, (long long)g.M, g.N, g.K, batch);
  const bool defer = g.d.a_stats || g.d.r_stats || g.d.o_stats;
  // the stage DMA as buffer loads (BufDma): K32-panel operands (the engine's launches) whose byte extents fit a 32-bit descriptor
  const bool buf_dma = g_buf_dma && g.a_panel && g.w_panel &&
#ifdef MH_ABLATE
                       !(g.dbg & 31) &&
#endif
                       mh_panel_desc_fits(g.K / 32, g.lda) && mh_panel_desc_fits(g.K / 32, g.ldw);
#define MH_LAUNCH_BIG(EPI_, ACT_, BITS_)                                                                             \
  do {                                                                                                                \
    if (buf_dma) MH_LAUNCH((gemm_big_kernel<C, EPI_, ACT_, (BITS_) | 16384>), grid, block, 0, s, g);                  \
    else MH_LAUNCH((gemm_big_kernel<C, EPI_, ACT_, (BITS_)>), grid, block, 0, s, g);                                  \
  } while (0)
  if constexpr (EPI == 1) {
    if (defer) {
      if constexpr (C::NW == 4) {
        MH_CHECK_ARG(g.d.a_stats && !g.d.r_stats && !g.d.o_stats, "gemm_qkv: deferred LayerNorm applies to the A operand only");
        MH_LAUNCH_BIG(1, MH_ACT_NONE, 128);
      } else { mh_set_error("gemm: deferred LayerNorm needs the 256x128 tile"); return MH_ERR_UNSUPPORTED; }
    }
    // q / k leave with ordinary stores: the attention kernel reads them back at once (round 2, after the epilogue restructuring:
    // +0.9 % steps/s over streaming stores, tools/ab_step.py plain_stores 0 1; round 1 had measured the opposite); bit 0 = streaming
#ifdef MH_ABLATE
    else if (g_plain_stores & 1) MH_LAUNCH((gemm_big_kernel<C, 1, MH_ACT_NONE>), grid, block, 0, s, g);
#endif
    else MH_LAUNCH_BIG(1, MH_ACT_NONE, 32);
  } else if constexpr (EPI == 3) {
    if (g.drop.thr || g.pre_out) {   // the training build: dropout (p may be 0) + the un-normalised rows kept for the backward
      if constexpr (C::BN == 512 && C::PP) MH_LAUNCH_BIG(3, MH_ACT_NONE, 64);
      else { mh_set_error("gemm: the dropout + LayerNorm epilogue is built for the 128x512 tile only"); return MH_ERR_UNSUPPORTED; }
    } else MH_LAUNCH_BIG(3, MH_ACT_NONE, 0);
  } else {
#ifdef MH_ABLATE
    if (g.dbg & 31) {   // timing-only ablations (tools/gemm_bench.py): 1 no DMA, 2 no MFMA, 4 no epilogue, 8 no LDS reads
      switch (g.dbg & 31) {
        case 1: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 1>), grid, block, 0, s, g); break;
        case 2: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 2>), grid, block, 0, s, g); break;
        case 4: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 4>), grid, block, 0, s, g); break;
        case 5: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 5>), grid, block, 0, s, g); break;
        case 6: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 6>), grid, block, 0, s, g); break;
        case 12: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 12>), grid, block, 0, s, g); break;
        case 13: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 13>), grid, block, 0, s, g); break;
        case 20: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 20>), grid, block, 0, s, g); break;
        case 28: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 28>), grid, block, 0, s, g); break;
        case 3: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, 2048>), grid, block, 0, s, g); break;      // bias + GELU, no stores
        case 7: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, 2049>), grid, block, 0, s, g); break;      // ... and no stage DMA
        case 9: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 2048>), grid, block, 0, s, g); break;          // bias only, no stores
        case 10: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 4096 + 4>), grid, block, 0, s, g); break;     // no epilogue, no W pieces
        default: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 14>), grid, block, 0, s, g); break;
      }
    } else
#endif
    if (defer) {
      if constexpr (C::NW == 4) {   // the operand combinations a post-LN encoder layer needs (engine.hip)
        const int da = g.d.a_stats ? 1 : 0, dr = g.d.r_stats ? 1 : 0, dd = g.d.o_stats ? 1 : 0;
        MH_CHECK_ARG(!g.act_grad && !g.out_f32 && !g.pre_out && (!dr || g.residual), "gemm: a deferred-LayerNorm launch has no activation gradient, fp32 or second output, and a raw residual needs the residual");
        if (da && !dr && !dd && g.act == MH_ACT_GELU_ERF) MH_LAUNCH_BIG(0, MH_ACT_GELU_ERF, 128);   // FFN1
        else if (da && !dr && !dd && g.act == MH_ACT_TANH) MH_LAUNCH_BIG(0, MH_ACT_TANH, 128);      // (down-projection)
        else if (!da && !dr && dd && g.act == MH_ACT_NONE) MH_LAUNCH_BIG(0, MH_ACT_NONE, 512);      // first attention-output dense
        else if (!da && dr && dd && g.act == MH_ACT_NONE) MH_LAUNCH_BIG(0, MH_ACT_NONE, 768);       // dense + raw residual -> raw rows
        else if (!da && dr && !dd && g.act == MH_ACT_NONE) MH_LAUNCH_BIG(0, MH_ACT_NONE, 256);      // last FFN output dense
        else { mh_set_error("gemm: unsupported deferred-LayerNorm operand combination (a=%d r=%d o=%d act=%d)", da, dr, dd, g.act); return MH_ERR_UNSUPPORTED; }
      } else { mh_set_error("gemm: deferred LayerNorm needs the 256x128 tile"); return MH_ERR_UNSUPPORTED; }
    } else {
      // the epilogue's form, where it is one of the fixed ones (see gemm_big_kernel: FORM); everything else takes the generic epilogue
      int form = 0;
      if (!g.out_f32 && !g.drop.thr) {
        if (!g.residual && !g.act_grad && !g.pre_out) form = 1;
        else if (g.residual && !g.act_grad && !g.pre_out) form = 2;
        else if (g.residual && g.act_grad == MH_ACT_DERIV && !g.pre_out) form = 4;
        else if (!g.residual && !g.act_grad && g.pre_out && g.pre_kind == 1 && g.act == MH_ACT_GELU_ERF) form = 8;
      }
      switch (g.act) {
      case MH_ACT_TANH:
        if (form == 1) MH_LAUNCH_BIG(0, MH_ACT_TANH, 1 << 16);
        else MH_LAUNCH_BIG(0, MH_ACT_TANH, 0);
        break;
      case MH_ACT_GELU_ERF:
#ifdef MH_ABLATE
        if (g_plain_stores & 2) MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_GELU_ERF, 32>), grid, block, 0, s, g);
        else
#endif
        if (form == 1) MH_LAUNCH_BIG(0, MH_ACT_GELU_ERF, 1 << 16);
        else if (form == 8) MH_LAUNCH_BIG(0, MH_ACT_GELU_ERF, 8 << 16);
        else MH_LAUNCH_BIG(0, MH_ACT_GELU_ERF, 0);
        break;
      case MH_ACT_SILU: MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_SILU>), grid, block, 0, s, g); break;
      default:
        if (g.drop.thr) MH_LAUNCH((gemm_big_kernel<C, 0, MH_ACT_NONE, 64>), grid, block, 0, s, g);
        else if (form == 1) MH_LAUNCH_BIG(0, MH_ACT_NONE, 1 << 16);
        else if (form == 2) MH_LAUNCH_BIG(0, MH_ACT_NONE, 2 << 16);
        else if (form == 4) MH_LAUNCH_BIG(0, MH_ACT_NONE, 4 << 16);
        else MH_LAUNCH_BIG(0, MH_ACT_NONE, 0);
        break;
      }
    }
  }
#undef MH_LAUNCH_BIG
  MH_CHECK_LAUNCH();
  return MH_OK;
}

}  // namespace mhgemm
