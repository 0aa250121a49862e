// gemm_args.h - what the GEMM objects share: the kernel argument structs, the big-tile configurations, apply_act and the host functions
// that cross an object boundary (the stage-DMA, wait-count and descriptor idioms: lds_dma.h).
//   gemm.hip           entry points, the dispatcher launch<EPI>, the 128x128 kernel (gemm_kernel), the nearest-embedding score path
//   gemm_big.h         the big-tile kernel (gemm_big_kernel) and launch_big<Cfg, EPI>, explicitly instantiated - once each - by
//   gemm_big_std.hip   256x128, EPI 0      gemm_big_wide.hip  256x256, EPI 0
//   gemm_big_qkv.hip   both, EPI 1         gemm_big_ln.hip    the full-row tiles, EPI 3
//   gemm_strip.hip     the column-strip kernel (gemm_strip.h) and, debug library only, the carried-epilogue experiment (gemm_carry.h)
//   gemm_dw.hip        the weight-gradient kernel (gemm_tn_kernel)
// The shared types sit in a NAMED namespace (an anonymous-namespace type is a different type in every object); its visibility is hidden, so
// nothing of it is exported from the library.
#pragma once
#include <type_traits>

#include "lds_dma.h"

int mh_drop_args(const mh_dropout* d, DropArgs* out);   // dropout.hip

namespace mhgemm __attribute__((visibility("hidden"))) {

// Deferred LayerNorm (bf16 throughput path): a dense + residual GEMM writes its RAW pre-LayerNorm rows plus per-row partial
// statistics (one (sum, sum of squares) pair per 128-column tile), and the consumers apply the normalisation themselves:
//   * as A operand:  LN(y) W^T + b = rstd_r ((y W'^T)_rc - mean_r c1_c) + c2_c  with W' = gamma o W (folded once, engine arena),
//     c1_c = sum_k W'_ck, c2_c = sum_k beta_k W_ck + b_c - the row scale / shift runs in the epilogue, on the accumulators;
//   * as residual:   (y - mean_r) rstd_r gamma_c + beta_c, element by element in the epilogue.
// No tile then needs to own complete rows: every GEMM of a layer runs on the 256x128 tile at two blocks per CU (d_model 768
// included, which has no full-row tile), and the LayerNorm kernels / epilogues disappear.
struct DeferArgs {
  const float* a_stats; int a_slots;   // A rows are raw: [M][a_slots][2] partial (sum, sumsq); g.bias then holds c2
  const float* c1;                     // [N] sum_k W'[c][k]
  const float* r_stats; int r_slots;   // residual rows are raw
  const float* r_gamma; const float* r_beta;
  float* o_stats; int o_slots;         // write the output rows' partial statistics, slot = column tile (n0 / BN)
  float inv_h, eps;                    // 1 / (normalised width), LayerNorm eps
};

struct GemmArgs {
  const void* A; int64_t lda;
  const void* W; int64_t ldw;
  const float* bias;
  const void* residual; int64_t ldr;
  void* out; int64_t ldo;
  int out_f32;
  int64_t M; int N; int K;
  int act;
  // QKV scatter
  void* q; void* k; void* vt;
  void* pre_out;   // EPI 0 with an activation (big tile): also store the pre-activation (bias added) here, same layout as out
  int64_t ldp; int p_panel;   // EPI 3 (training form): pre_out's own layout (row pitch / panel rows; 0 = as `out`: ldo, row-major)
  int act_grad;    // EPI 0 (big tile): `residual` holds a PRE-activation and the result is multiplied by act'(it) instead of added to
  int L, H, nh, dh;
  // EPI 2 (nearest-embedding scores): aux[col] = |W_col|^2, rown[row] = |x_row|^2, partial best per (row, slot)
  const float* aux; const float* rown; float* pbest; int32_t* pidx; int nslots;
  int a_panel, w_panel, o_panel, r_panel;  // operand stored as K32 panels: [cols/32][ld rows][32]
  int64_t sA, sW, sO, sR;  // batch strides in elements (grid.y = batch index)
  const float* ln_gamma; const float* ln_beta; float ln_eps;   // EPI 3
  int dbg;  // timing-only ablation bits (mh_gemm_set_debug): 1 no DMA, 2 no MFMA, 4 no stores
  int ntiles;    // persistent big-tile launch: ntiles output tiles walked by gridDim.x blocks
  int vt_perm;   // QKV scatter: V^T keys in the P-operand order of mh_attention_stream_fwd (middle groups of 4 swapped per 16)
  int pre_kind;  // what pre_out receives: 0 the pre-activation, 1 act'(pre) (GELU: gelu_erf_fast8_dgelu)
  float q_scale; // QKV scatter (big tile): the query columns are stored multiplied by this (0 = unscaled): softmax scale x log2(e) for mh_attention_stream_fwd_prescaled
  DeferArgs d;   // DBG bit 128 kernels only
  DropArgs drop; // EPI 0: train-mode dropout of (A W^T + bias) before the residual is added (thr == 0: off)
};

template <typename T>
__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case MH_ACT_TANH: return sizeof(T) == 2 ? tanh_fast(v) : tanhf(v);
    case MH_ACT_GELU_ERF: return sizeof(T) == 2 ? gelu_erf_fast(v) : gelu_erf(v);
    case MH_ACT_SILU: return silu(v);
    default: return v;
  }
}

// Big-tile configurations (gemm_big.h describes the kernels)
template <int BM_, int BN_, int WM_, int WN_, int NST_, bool PP_ = false>
struct BigCfg {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, NST = NST_;
  static constexpr bool PP = PP_;   // ping-pong main loop (two wave groups half a K-step apart)
  static constexpr int PRO = PP_ ? NST_ - 1 : NST_;   // stages a main loop has in flight before its first K-step
  static constexpr int NW = WM * WN, THREADS = NW * 64;
  static constexpr int TI = BM / WM / 16, TJ = BN / WN / 16;
  static constexpr int STAGE = (BM + BN) * 64;
  // DMA pieces (16 rows x 64 B) per wave and stage.  A tile with fewer A pieces than waves (BM 64 on 8 waves) still gives every
  // wave one: the upper waves re-load the lower waves' pieces (identical bytes to the same LDS address), so that every wave's
  // vmcnt arithmetic stays the same
  static constexpr int APIECES = BM / 16;
  static constexpr int PA = (APIECES + NW - 1) / NW, PW = BN / 16 / NW, PIECES = PA + PW;
  static_assert(PA >= 1 && PW >= 1 && TJ % 4 == 0 && NST >= 3 && (APIECES % NW == 0 || NW % APIECES == 0), "unsupported big-tile configuration");
};
using CfgStd = BigCfg<256, 128, 2, 2, 3>;
using CfgWide = BigCfg<256, 256, 2, 4, 4>;
using CfgRow = BigCfg<128, 512, 2, 4, 3>;
using CfgWidePP = BigCfg<256, 256, 2, 4, 4, true>;
using CfgRowPP = BigCfg<128, 512, 2, 4, 3, true>;
using CfgRow64 = BigCfg<64, 512, 1, 8, 3>;   // full-row tile over 64 rows: twice the blocks of CfgRow (short K: the epilogue dominates)
constexpr int B2K = 32;

#ifndef MH_PLAIN_STORES_DEFAULT
#define MH_PLAIN_STORES_DEFAULT 0
#endif
// round 5: K32-panel launches (the engine's) issue their stage DMA as buffer loads (BufDma above): bit-identical results, no vector address
// arithmetic per piece.  A/B: mh_gemm_set_buf_dma(0) = global_load_lds with per-piece 64-bit addresses (rounds 1 - 4)
inline MH_KNOB(int, g_buf_dma, 1);
inline MH_KNOB(int, g_plain_stores, MH_PLAIN_STORES_DEFAULT);   // A/B: bit 0 QKV streaming instead of ordinary stores, bit 1 dense+GELU ordinary instead of streaming stores; bit 2: full-row tile without ping-pong; bits 3 / 4: 64-row full-row tile

// ---- host functions defined in one object and called from another
bool big_tile_ok(const GemmArgs& g);       // gemm.hip
template <class C, int EPI> int launch_big(const GemmArgs& g0, hipStream_t s, int batch);   // gemm_big.h; instantiated by gemm_big_*.hip
bool strip_ok(const GemmArgs& g);          // gemm_strip.h (gemm_big_std.hip)
int launch_strip(const GemmArgs& g, hipStream_t s);
#ifdef MH_ABLATE
int launch_carry(const GemmArgs& g0, int variant, hipStream_t s);   // gemm_carry.h (gemm_big_std.hip)
#endif

}  // namespace mhgemm
