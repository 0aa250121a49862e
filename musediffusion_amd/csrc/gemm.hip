// GEMM family: out = act(A W^T + bias) [+ residual]  and the fused QKV projection with head scatter.
//
// CDNA4 mapping (one design for both element types, 128x128 block tile, 4 waves as 2(M) x 2(N),
// each wave a 64x64 sub-tile = 4x4 MFMA tiles of 16x16):
//   bf16: v_mfma_f32_16x16x32_bf16, K-tile 64.  LDS rows are 128 B; the 16-B chunk c of row r lives
//         at chunk (c ^ (r & 7)) so that the ds_read_b128 fragment reads (16 rows x 2 chunks per
//         16-lane group) hit 16 distinct 16-B slots of the 256-B bank row: conflict-free.
//         Staging is register-staged (global_load_dwordx4 -> ds_write_b128).
//   f32:  v_mfma_f32_16x16x4_f32 (exact fp32 fma chain), K-tile 16.  The k index served by lane
//         group g in instruction s is 4g+s for BOTH operands, so one ds_read_b128 per tile row
//         feeds four MFMAs.  LDS rows are padded to 96 B (slot = 6*row + g: conflict-free).
//   Both: double-buffered LDS, one barrier per K-tile; the epilogue stages each wave's
//         accumulators through LDS so that bias / activation / residual / stores work on 8
//         contiguous columns per lane (16-B bf16 stores).
// nn.Linear convention: W is [N, K] row-major ("B^T"), which is exactly the k-contiguous layout
// the MFMA B operand wants, so no weight transposition happens anywhere.
#include "gemm_args.h"

using namespace mhgemm;

namespace {

template <typename T> struct Tile;
template <> struct Tile<bf16> { static constexpr int BK = 64, ROWB = 128, CHUNKS = 8; };
template <> struct Tile<float> { static constexpr int BK = 16, ROWB = 80, CHUNKS = 4; };

constexpr int BM = 128, BN = 128, CS_LD = 68;

template <typename T, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs g) {
  using TT = Tile<T>;
  constexpr int BK = TT::BK, ROWB = TT::ROWB, CHUNKS = TT::CHUNKS;
  constexpr int TILE_BYTES = 128 * ROWB;
  constexpr int NCH = (128 * CHUNKS) / 256;  // 16-B chunks per thread per operand tile
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (g.N + BN - 1) / BN;
  const int bid = mh_xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (int64_t)(bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const T* __restrict__ A = reinterpret_cast<const T*>(g.A) + (int64_t)blockIdx.y * g.sA;
  const T* __restrict__ W = reinterpret_cast<const T*>(g.W) + (int64_t)blockIdx.y * g.sW;
  const int nk = g.K / BK;
  constexpr int EPC = 16 / sizeof(T);  // elements per 16-B chunk

  // ---- per-thread staging coordinates (fixed over the K loop)
  const T* srcA[NCH];
  const T* srcW[NCH];
  int ldsoff[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int row, c, off;
    const int qd = tid + 256 * j;
    row = qd / CHUNKS;
    c = qd % CHUNKS;
    if constexpr (sizeof(T) == 2) off = row * ROWB + ((c ^ (row & 7)) << 4);
    else off = row * ROWB + (c << 4);
    int64_t ra = m0 + row; if (ra >= g.M) ra = g.M - 1;
    int rw = n0 + row; if (rw >= g.N) rw = g.N - 1;
    srcA[j] = A + ra * g.lda + c * EPC;
    srcW[j] = W + (int64_t)rw * g.ldw + c * EPC;
    ldsoff[j] = off;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 stA[NCH], stW[NCH];  // staging registers

  auto issue = [&](int kt, int) {
    const int koff = kt * BK;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      stA[j] = *reinterpret_cast<const f32x4*>(srcA[j] + koff);
      stW[j] = *reinterpret_cast<const f32x4*>(srcW[j] + koff);
    }
  };
  auto commit = [&](int buf) {
    char* base = smem + buf * 2 * TILE_BYTES;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      *reinterpret_cast<f32x4*>(base + ldsoff[j]) = stA[j];
      *reinterpret_cast<f32x4*>(base + TILE_BYTES + ldsoff[j]) = stW[j];
    }
  };

  issue(0, 0);
  commit(0);
  __syncthreads();

  const int fr = lane & 15, fg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) issue(kt + 1, cur ^ 1);
    const char* As = smem + cur * 2 * TILE_BYTES;
    const char* Ws = As + TILE_BYTES;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 a[4], b[4];
        const int chunk = kk * 4 + fg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ra = wm * 64 + i * 16 + fr;
          a[i] = *reinterpret_cast<const bf16x8*>(As + ra * ROWB + ((chunk ^ (ra & 7)) << 4));
          const int rb = wn * 64 + i * 16 + fr;
          b[i] = *reinterpret_cast<const bf16x8*>(Ws + rb * ROWB + ((chunk ^ (rb & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    } else {
      f32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = *reinterpret_cast<const f32x4*>(As + (wm * 64 + i * 16 + fr) * ROWB + (fg << 4));
        b[i] = *reinterpret_cast<const f32x4*>(Ws + (wn * 64 + i * 16 + fr) * ROWB + (fg << 4));
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) commit(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: each wave stages 32 rows x 64 cols of fp32 at a time in its own LDS region
  float* Cs = reinterpret_cast<float*>(smem) + wave * (32 * CS_LD);
  const bool vec_ok = (g.ldo % 8 == 0) && (g.ldr % 8 == 0);
  T* outT = reinterpret_cast<T*>(g.out) + (int64_t)blockIdx.y * g.sO;
  float* outF = reinterpret_cast<float*>(g.out) + (int64_t)blockIdx.y * g.sO;
  const T* res = g.residual ? reinterpret_cast<const T*>(g.residual) + (int64_t)blockIdx.y * g.sR : nullptr;
  const int wcol0 = n0 + wn * 64;                      // first column of this wave's region
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int il = 0; il < 2; ++il)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          Cs[(il * 16 + fg * 4 + r) * CS_LD + j * 16 + fr] = acc[2 * p + il][j][r];
    __syncthreads();
    const int64_t wrow0 = m0 + wm * 64 + p * 32;
    if constexpr (EPI == 1) {
      // QKV scatter.  A wave's 64 columns lie inside one of Q | K | V and inside one head block
      // boundary multiple (H % 64 == 0), so `which` is wave-uniform.
      const int which = wcol0 / g.H;
      if (which < 2) {
        T* dst = reinterpret_cast<T*>(which == 0 ? g.q : g.k);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int idx = it * 64 + lane, rl = idx >> 3, c8 = (idx & 7) * 8;
          const int64_t row = wrow0 + rl;
          const int col = wcol0 + c8;
          if (row < g.M && col < g.N) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = Cs[rl * CS_LD + c8 + e] + g.bias[col + e];
            const int c = col - which * g.H, head = c / g.dh, d = c % g.dh;
            const int64_t b = row / g.L, l = row % g.L;
            store8(dst + ((b * g.nh + head) * g.L + l) * g.dh + d, v);
          }
        }
      } else {
        T* dst = reinterpret_cast<T*>(g.vt);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int idx = it * 64 + lane, cl = idx & 63, rg = idx >> 6;
          const int64_t row = wrow0 + rg * 8;
          const int col = wcol0 + cl;
          if (row < g.M && col < g.N) {
            float v[8];
            const float bv = g.bias[col];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = Cs[(rg * 8 + e) * CS_LD + cl] + bv;
            const int c = col - 2 * g.H, head = c / g.dh, d = c % g.dh;
            const int64_t b = row / g.L, l = row % g.L;
            store8(dst + ((b * g.nh + head) * g.dh + d) * g.L + l, v);
          }
        }
      }
    } else if constexpr (EPI == 2) {
      // rounding scores (models/rounding.py:21-28): -(clamp((|W_v|^2 + |x_n|^2) - 2 x.W_v, 0)); every row keeps
      // the best (score, first index) of this wave's 64 columns -> one partial per (row, column-slot)
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = it * 64 + lane, rl = idx >> 3, c8 = (idx & 7) * 8;
        const int64_t row = wrow0 + rl;
        const int col = wcol0 + c8;
        float best = -INFINITY;
        int bi = 0x7fffffff;
        if (row < g.M) {
          const float xn = g.rown[row];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (col + e < g.N) {
              float dist = (g.aux[col + e] + xn) - 2.0f * Cs[rl * CS_LD + c8 + e];
              dist = fmaxf(dist, 0.0f);
              const float sc = -dist;
              if (sc > best) { best = sc; bi = col + e; }
            }
          }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
          const float so = __shfl_xor(best, off, 64);
          const int io = __shfl_xor(bi, off, 64);
          if (so > best || (so == best && io < bi)) { best = so; bi = io; }
        }
        if ((lane & 7) == 0 && row < g.M) {
          const int slot = (n0 / BN) * 2 + wn;
          g.pbest[row * g.nslots + slot] = best;
          g.pidx[row * g.nslots + slot] = bi;
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = it * 64 + lane, rl = idx >> 3, c8 = (idx & 7) * 8;
        const int64_t row = wrow0 + rl;
        const int col = wcol0 + c8;
        if (row < g.M && col < g.N) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = Cs[rl * CS_LD + c8 + e];
          const int nv = (g.N - col) < 8 ? (g.N - col) : 8;
          if (g.bias) {
#pragma unroll
            for (int e = 0; e < 8; ++e) if (e < nv) v[e] += g.bias[col + e];
          }
          if (g.act != MH_ACT_NONE) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = apply_act<T>(v[e], g.act);
          }
          if (g.drop.thr) {   // HF BertSelfOutput / BertOutput: dense -> dropout -> (+ input) (N % 8 == 0: checked by the entry point)
            const uint32_t km = drop_keep8_at(g.drop, (uint64_t)row * g.N + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (km >> e) & 1u ? v[e] * g.drop.rscale : 0.f;
          }
          if (nv == 8 && vec_ok) {
            if (res) {
              float rv[8];
              load8(res + row * g.ldr + col, rv);
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] += rv[e];
            }
            if (g.out_f32) store8(outF + row * g.ldo + col, v);
            else store8(outT + row * g.ldo + col, v);
          } else {
            for (int e = 0; e < nv; ++e) {
              float x = v[e];
              if (res) x += to_f32(res[row * g.ldr + col + e]);
              if (g.out_f32) outF[row * g.ldo + col + e] = x;
              else outT[row * g.ldo + col + e] = from_f32<T>(x);
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

MH_KNOB(int, g_dbg, 0);
MH_KNOB(int, g_variant, 2);  // bf16 kernel choice: 0 the 128x128 register-staged tile everywhere (the fallback of shapes the big tiles do not serve), 2 big tiles (256x128; 256x256 for row-major launches that fill the chip with it), 4 big 256x256

}  // namespace

namespace mhgemm __attribute__((visibility("hidden"))) {

bool big_tile_ok(const GemmArgs& g) {
  // N % 8 == 0: a lane's 8 output columns are all valid; an fp32 row-major output may end on a half group (N % 4 == 0, e.g. the
  // released checkpoints' E = 500 down-projection): the epilogue stores only the first four of the last lane's columns
  const bool n_ok = g.N % 8 == 0 || (g.out_f32 && g.N % 4 == 0 && g.act_grad == 0 && !g.residual && !g.pre_out && !g.q && !g.ln_gamma && !g.drop.thr);
  return n_ok && g.K % B2K == 0 && (g.o_panel || g.ldo % 8 == 0 || (g.out_f32 && g.ldo % 4 == 0)) &&
         (g.r_panel || g.ldr % 8 == 0);
}

}  // namespace mhgemm

namespace {
// The wide (256x256, one block per CU) tile moves 1.5x fewer operand bytes per flop, but measured inside the captured step
// (tools/ab_step.py, two graph branches) the 256x128 tile is 1.2% faster: at two blocks per CU the blocks of two
// concurrently running kernels share a CU, which is what the branches are for.  Wide / ping-pong stay selectable (4 / 5).
// Round 3: launches with ROW-MAJOR operands (the training tape, direct callers: one GEMM on the chip at a time) take the wide tile
// when it still gives every CU a block - bench.py --workload train -2.1 % (tools/ab_train.py gemm_variant 2 4); the engine's
// K32-panel launches (two concurrent branches) keep the 256x128 tile.  mh_gemm_set_auto_wide(0) switches the rule off.
MH_KNOB(int, g_auto_wide, 1);
MH_KNOB(int, g_wide_roles, 0);   // A/B (mh_gemm_set_wide_roles): panel launches on the 256x256 tile by role: bit 0 dense + GELU, bit 1 QKV scatter, bit 2 the rest
bool want_wide(const GemmArgs& g, int batch) {
  if (g.N % 256 != 0) return false;
  if (g_variant >= 4) return true;
  if (g_wide_roles && (g.a_panel || g.w_panel)) {
    const int role = g.act == MH_ACT_GELU_ERF ? 1 : (g.q ? 2 : 4);
    if (g_wide_roles & role) return true;
  }
  if (g_variant != 2 || !g_auto_wide || batch != 1) return false;
  if (g.a_panel || g.w_panel || g.o_panel || g.r_panel || g.q) return false;
  return (int64_t)ceil_div(g.M, 256) * (g.N / 256) >= mh_device_cus();
}

// round 6: dense + bias + GELU of K32 panels (the sampler's FFN1) on the column-strip kernel; A/B: mh_gemm_set_strip(0) = gemm_big_kernel
MH_KNOB(int, g_strip, 1);

template <int EPI>
int launch(const GemmArgs& g, int dtype, hipStream_t s, int batch = 1) {
  const int64_t tiles = (int64_t)ceil_div(g.M, BM) * ceil_div(g.N, BN);
  MH_CHECK_ARG(tiles > 0 && tiles < (1ll << 31), "gemm: bad grid (M=%lld N=%d)", (long long)g.M, g.N);
  MH_CHECK_ARG(batch >= 1 && batch <= 65535, "gemm: batch %d out of range", batch);
  dim3 grid((unsigned)tiles, (unsigned)batch), block(256);
  mh_prof_note("tile=128x128 epi=%d act=%d M=%lld N=%d K=%d batch=%d dtype=%d", EPI, g.act, (long long)g.M, g.N, g.K, batch, dtype);
  if (dtype == MH_BF16) {
    MH_CHECK_ARG((g.a_panel || g.lda % 8 == 0) && (g.w_panel || g.ldw % 8 == 0), "gemm(bf16): lda/ldw must be multiples of 8");
    const bool any_panel = g.a_panel || g.w_panel || g.o_panel || g.r_panel;
    const bool big_ok = big_tile_ok(g);
    MH_CHECK_ARG(!any_panel || (big_ok && g_variant >= 2), "gemm: panel layouts need the big-tile bf16 kernel");
    MH_CHECK_ARG(g.K > 0 && (g.K % 64 == 0 || (g.K % B2K == 0 && big_ok && g_variant >= 2)),
                 "gemm(bf16): K=%d must be a positive multiple of 64 (32 with the big-tile kernel)", g.K);
    if (EPI != 2 && g_variant >= 2 && big_ok) {
      if constexpr (EPI == 2) return MH_OK;
      // QKV scatter: a wave's columns must not straddle the q/k/v boundary (H % 64 == 0 for the wide tile)
      else {
        if constexpr (EPI == 0) {
          if (g_strip && batch == 1 && g_variant == 2 && strip_ok(g)) return launch_strip(g, s);
        }
        if (g.d.a_stats || g.d.r_stats || g.d.o_stats) return launch_big<CfgStd, EPI>(g, s, batch);   // deferred LayerNorm: 256x128 only
        if (want_wide(g, batch) && (EPI != 1 || g.H % 64 == 0)) return launch_big<CfgWide, EPI>(g, s, batch);
        return launch_big<CfgStd, EPI>(g, s, batch);
      }
    } else {
      MH_LAUNCH((gemm_kernel<bf16, EPI>), grid, block, 0, s, g);
    }
  } else if (dtype == MH_F32) {
    MH_CHECK_ARG(!(g.a_panel || g.w_panel || g.o_panel || g.r_panel), "gemm(f32): panel layouts are bf16 only");
    MH_CHECK_ARG(g.K % 16 == 0 && g.K > 0, "gemm(f32): K=%d must be a positive multiple of 16", g.K);
    MH_CHECK_ARG(g.lda % 4 == 0 && g.ldw % 4 == 0, "gemm(f32): lda/ldw must be multiples of 4");
    MH_LAUNCH((gemm_kernel<float, EPI>), grid, block, 0, s, g);
  } else {
    MH_CHECK_ARG(false, "gemm: unknown dtype %d", dtype);
  }
  MH_CHECK_LAUNCH();
  return MH_OK;
}

}  // namespace

extern "C" int mh_gemm_bias_res_ln_supported(int N) { return N == 128 || N == 256 || N == 512; }

#ifdef MH_ABLATE
extern "C" int mh_gemm_set_plain_stores(int mask) {
  g_plain_stores = mask;
  return MH_OK;
}
#endif

#ifdef MH_ABLATE
extern "C" int mh_gemm_set_strip(int on) {
  g_strip = on != 0;
  return MH_OK;
}
#endif

#ifdef MH_ABLATE
extern "C" int mh_gemm_set_buf_dma(int on) {
  g_buf_dma = on != 0;
  return MH_OK;
}
#endif

#ifdef MH_ABLATE
extern "C" int mh_gemm_set_debug(int bits) {
  g_dbg = bits & 127;
  return MH_OK;
}
#endif

#ifdef MH_ABLATE
extern "C" int mh_gemm_set_wide_roles(int mask) {
  g_wide_roles = mask;
  return MH_OK;
}
#endif
#ifdef MH_ABLATE
extern "C" int mh_gemm_set_auto_wide(int on) {
  g_auto_wide = on ? 1 : 0;
  return MH_OK;
}
#endif

#ifdef MH_ABLATE
extern "C" int mh_gemm_set_variant(int variant) {
  MH_CHECK_ARG(variant == 0 || variant == 2 || variant == 4, "gemm_set_variant: variant must be 0, 2 or 4");
  g_variant = variant;
  return MH_OK;
}
#endif

#ifdef MH_ABLATE
// experiment (gemm_carry.h): dense + bias + GELU of K32-panel operands into a K32-panel output with the previous tile's epilogue carried
extern "C" int mh_gemm_ffn1_carry(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out, int64_t ldo,
                                  int64_t M, int N, int K, int variant, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && bias && out && M > 0 && N > 0, "gemm_ffn1_carry: null pointer / empty problem");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.out = out; g.ldo = ldo; g.ldr = 8;
  g.M = M; g.N = N; g.K = K; g.act = MH_ACT_GELU_ERF; g.a_panel = g.w_panel = g.o_panel = 1;
  return launch_carry(g, variant, (hipStream_t)stream);
}
#endif

extern "C" int mh_gemm_bias_act(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                                const void* residual, int64_t ldr, void* out, int64_t ldo, int out_f32,
                                int64_t M, int N, int K, int act, int dtype, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out, "gemm: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0, "gemm: empty problem M=%lld N=%d", (long long)M, N);
  MH_CHECK_ARG(act >= MH_ACT_NONE && act <= MH_ACT_SILU, "gemm: unknown activation %d", act);
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
  g.residual = residual; g.ldr = residual ? ldr : 8; g.out = out; g.ldo = ldo; g.out_f32 = out_f32;
  g.M = M; g.N = N; g.K = K; g.act = act; g.dbg = g_dbg & 127;
  return launch<0>(g, dtype, (hipStream_t)stream);
}

extern "C" int mh_gemm_bias_act_ex(const void* A, int64_t lda, int a_panel, const void* W, int64_t ldw, int w_panel,
                                   const float* bias, const void* residual, int64_t ldr, int r_panel, void* out,
                                   int64_t ldo, int o_panel, int out_f32, int64_t M, int N, int K, int act, int dtype,
                                   mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out, "gemm: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0, "gemm: empty problem M=%lld N=%d", (long long)M, N);
  MH_CHECK_ARG(act >= MH_ACT_NONE && act <= MH_ACT_SILU, "gemm: unknown activation %d", act);
  MH_CHECK_ARG(!(o_panel && out_f32), "gemm: fp32 output is row-major only");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
  g.residual = residual; g.ldr = residual ? ldr : 8; g.out = out; g.ldo = ldo; g.out_f32 = out_f32;
  g.M = M; g.N = N; g.K = K; g.act = act; g.dbg = g_dbg & 127;
  g.a_panel = a_panel; g.w_panel = w_panel; g.o_panel = o_panel; g.r_panel = residual ? r_panel : 0;
  return launch<0>(g, dtype, (hipStream_t)stream);
}

namespace {
int fill_defer(const mh_ln_defer* d, GemmArgs& g, const char* who) {
  if (!d) return MH_OK;
  MH_CHECK_ARG(d->h_norm > 0 && d->eps >= 0.f, "%s: deferred LayerNorm needs the normalised width and eps", who);
  MH_CHECK_ARG(!d->a_stats || (d->c1 && d->a_slots > 0), "%s: a_stats needs c1 and a_slots", who);
  MH_CHECK_ARG(!d->r_stats || (d->r_gamma && d->r_beta && d->r_slots > 0 && g.residual), "%s: r_stats needs gamma, beta, r_slots and a residual", who);
  MH_CHECK_ARG(!d->o_stats || d->o_slots >= ceil_div(g.N, 128), "%s: o_slots must cover the %d column tiles", who, ceil_div(g.N, 128));
  g.d.a_stats = d->a_stats; g.d.a_slots = d->a_slots; g.d.c1 = d->c1;
  g.d.r_stats = d->r_stats; g.d.r_slots = d->r_slots; g.d.r_gamma = d->r_gamma; g.d.r_beta = d->r_beta;
  g.d.o_stats = d->o_stats; g.d.o_slots = d->o_slots;
  g.d.inv_h = 1.0f / (float)d->h_norm; g.d.eps = d->eps;
  return MH_OK;
}
}  // namespace

// mh_gemm_bias_act_ex in the K32-panel layout (all four operands) with deferred-LayerNorm operands (struct mh_ln_defer):
//   out = act(LN?(A) W^T + bias) [+ LN?(residual)], optionally writing the output rows' partial statistics.
extern "C" int mh_gemm_bias_act_defer(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const void* residual,
                                      int64_t ldr, void* out, int64_t ldo, int64_t M, int N, int K, int act, const mh_ln_defer* defer,
                                      mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out && bias, "gemm_bias_act_defer: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0 && N % 8 == 0 && K % B2K == 0, "gemm_bias_act_defer: bad problem M=%lld N=%d K=%d", (long long)M, N, K);
  MH_CHECK_ARG(act == MH_ACT_NONE || act == MH_ACT_TANH || act == MH_ACT_GELU_ERF, "gemm_bias_act_defer: activation %d", act);
  MH_CHECK_ARG(g_variant >= 2, "gemm_bias_act_defer: needs the big-tile bf16 kernel");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
  g.residual = residual; g.ldr = residual ? ldr : 8; g.out = out; g.ldo = ldo;
  g.M = M; g.N = N; g.K = K; g.act = act;
  g.a_panel = 1; g.w_panel = 1; g.o_panel = 1; g.r_panel = residual ? 1 : 0;
  int rc = fill_defer(defer, g, "gemm_bias_act_defer");
  if (rc) return rc;
  return launch<0>(g, MH_BF16, (hipStream_t)stream);
}

// out = LayerNorm(A W^T + bias + residual) * gamma + beta over complete rows: the block owns all N columns
// (N = 128, 256 or 512), so the normalisation runs on the accumulators (models/network.py:150 ->
// BertSelfOutput / BertOutput: dense -> dropout(eval: identity) -> LayerNorm(hidden + input))
extern "C" int mh_gemm_bias_res_ln(const void* A, int64_t lda, int a_panel, const void* W, int64_t ldw, int w_panel,
                                   const float* bias, const void* residual, int64_t ldr, int r_panel, const float* gamma,
                                   const float* beta, float eps, void* out, int64_t ldo, int o_panel, int64_t M, int N,
                                   int K, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out && bias && residual && gamma && beta, "gemm_bias_res_ln: null pointer");
  MH_CHECK_ARG(M > 0 && K > 0 && K % B2K == 0, "gemm_bias_res_ln: bad problem M=%lld K=%d", (long long)M, K);
  MH_CHECK_ARG(mh_gemm_bias_res_ln_supported(N), "gemm_bias_res_ln: N=%d must be 128, 256 or 512", N);
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
  g.residual = residual; g.ldr = ldr; g.out = out; g.ldo = ldo;
  g.M = M; g.N = N; g.K = K; g.act = MH_ACT_NONE;
  g.a_panel = a_panel; g.w_panel = w_panel; g.o_panel = o_panel; g.r_panel = r_panel;
  g.ln_gamma = gamma; g.ln_beta = beta; g.ln_eps = eps;
  MH_CHECK_ARG((a_panel || lda % 8 == 0) && (w_panel || ldw % 8 == 0) && big_tile_ok(g), "gemm_bias_res_ln: leading dimensions must be multiples of 8");
  hipStream_t s = (hipStream_t)stream;
  if (N == 128) return launch_big<CfgStd, 3>(g, s, 1);
  if (N == 256) return launch_big<CfgWidePP, 3>(g, s, 1);
  // one block per CU: the ping-pong main loop pays here (-4.5% step time, tools/ab_step.py); bit 2 of the A/B mask = plain loop
#ifdef MH_ABLATE
  if (g_plain_stores & 4) return launch_big<CfgRow, 3>(g, s, 1);
  if ((g_plain_stores & 16) || ((g_plain_stores & 8) && K <= 512)) return launch_big<CfgRow64, 3>(g, s, 1);   // A/B: 64-row full-row tile
#endif
  return launch_big<CfgRowPP, 3>(g, s, 1);
}

// out = dropout(A W^T + bias) + residual: the dense half of HF BertSelfOutput / BertOutput in train mode (the LayerNorm that
// follows stays a separate kernel on the training path).  Row-major operands; N % 8 == 0.  The keep mask of element (row, col)
// comes from Philox4x32-7 keyed by drop->seed at counter ((row N + col) / 8, drop->offset) - mh_dropout_fwd with the same
// descriptor re-creates it for the backward - or from drop->mask (tests).
extern "C" int mh_gemm_bias_dropout_res(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const void* residual,
                                        int64_t ldr, void* out, int64_t ldo, int64_t M, int N, int K, int dtype, const mh_dropout* drop,
                                        mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out, "gemm_bias_dropout_res: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0 && N % 8 == 0, "gemm_bias_dropout_res: bad problem M=%lld N=%d (N must be a multiple of 8)", (long long)M, N);
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
  g.residual = residual; g.ldr = residual ? ldr : 8; g.out = out; g.ldo = ldo;
  g.M = M; g.N = N; g.K = K; g.act = MH_ACT_NONE; g.dbg = 0;
  int rc = mh_drop_args(drop, &g.drop);
  if (rc) return rc;
  MH_CHECK_ARG(ldo % 8 == 0 && (!residual || ldr % 8 == 0), "gemm_bias_dropout_res: ldo / ldr must be multiples of 8");
  return launch<0>(g, dtype, (hipStream_t)stream);
}

// out = LayerNorm(pre) with pre = dropout(A W^T + bias) + residual, and pre itself (bf16-rounded, what the LayerNorm backward reads):
// BertSelfOutput / BertOutput in train mode as ONE kernel (N = 512, row-major bf16; drop may be null or p = 0)
extern "C" int mh_gemm_bias_dropout_res_ln(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const void* residual,
                                           int64_t ldr, const float* gamma, const float* beta, float eps, void* pre_out, void* out,
                                           int64_t ldo, int64_t M, int N, int K, const mh_dropout* drop, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out && pre_out && bias && residual && gamma && beta, "gemm_bias_dropout_res_ln: null pointer");
  MH_CHECK_ARG(M > 0 && K > 0 && K % B2K == 0 && N == 512, "gemm_bias_dropout_res_ln: needs N = 512 and K %% 32 == 0 (got N=%d K=%d)", N, K);
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
  g.residual = residual; g.ldr = ldr; g.out = out; g.ldo = ldo; g.pre_out = pre_out;
  g.M = M; g.N = N; g.K = K; g.act = MH_ACT_NONE;
  g.ln_gamma = gamma; g.ln_beta = beta; g.ln_eps = eps;
  int rc = mh_drop_args(drop, &g.drop);
  if (rc) return rc;
  MH_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && ldo % 8 == 0 && ldr % 8 == 0, "gemm_bias_dropout_res_ln: leading dimensions must be multiples of 8");
  return launch_big<CfgRowPP, 3>(g, (hipStream_t)stream, 1);
}

// act(A W^T + bias) -> out AND A W^T + bias -> pre_out in one pass (bf16, row-major, big-tile shapes only): the forward of
// a dense + activation layer under autograd, whose backward needs the pre-activation (training.py:_Linear)
extern "C" int mh_gemm_bias_act_pre(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* pre_out,
                                    void* out, int64_t ldo, int64_t M, int N, int K, int act, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out && pre_out, "gemm_bias_act_pre: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0 && act > MH_ACT_NONE && act <= MH_ACT_SILU, "gemm_bias_act_pre: bad problem / activation");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.ldr = 8; g.out = out; g.ldo = ldo;
  g.M = M; g.N = N; g.K = K; g.act = act; g.pre_out = pre_out;
  MH_CHECK_ARG(g_variant >= 2 && lda % 8 == 0 && ldw % 8 == 0 && big_tile_ok(g), "gemm_bias_act_pre: shape not served by the big-tile kernel");
  return launch<0>(g, MH_BF16, (hipStream_t)stream);
}

// mh_gemm_bias_act_pre for GELU with the DERIVATIVE in place of the pre-activation: dact_out = gelu'(A W^T + bias) (bf16), out = gelu(...).
// The backward multiplies by it (mh_gemm_act_grad with act = MH_ACT_DERIV) instead of evaluating gelu' again from the pre-activation.
extern "C" int mh_gemm_bias_act_dact(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* dact_out,
                                     void* out, int64_t ldo, int64_t M, int N, int K, int act, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out && dact_out, "gemm_bias_act_dact: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0 && act == MH_ACT_GELU_ERF, "gemm_bias_act_dact: bad problem / activation (GELU only)");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.ldr = 8; g.out = out; g.ldo = ldo;
  g.M = M; g.N = N; g.K = K; g.act = act; g.pre_out = dact_out; g.pre_kind = 1;
  MH_CHECK_ARG(g_variant >= 2 && lda % 8 == 0 && ldw % 8 == 0 && big_tile_ok(g), "gemm_bias_act_dact: shape not served by the big-tile kernel");
  return launch<0>(g, MH_BF16, (hipStream_t)stream);
}

// out = (A W^T) o act'(pre): the input-gradient GEMM of the layer AFTER an activation with the activation's own backward
// folded into its epilogue (bf16 row-major, big-tile shapes; act = tanh or erf-GELU)
extern "C" int mh_gemm_act_grad(const void* A, int64_t lda, const void* W, int64_t ldw, const void* pre, int64_t ld_pre, void* out,
                                int64_t ldo, int64_t M, int N, int K, int act, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && pre && out, "gemm_act_grad: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0 && (act == MH_ACT_TANH || act == MH_ACT_GELU_ERF || act == MH_ACT_DERIV), "gemm_act_grad: bad problem / activation");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.residual = pre; g.ldr = ld_pre; g.out = out; g.ldo = ldo;
  g.M = M; g.N = N; g.K = K; g.act = MH_ACT_NONE; g.act_grad = act;
  MH_CHECK_ARG(g_variant >= 2 && lda % 8 == 0 && ldw % 8 == 0 && big_tile_ok(g), "gemm_act_grad: shape not served by the big-tile kernel");
  return launch<0>(g, MH_BF16, (hipStream_t)stream);
}

// One descriptor for every bf16 dense launch of the training step (csrc/train_layer.hip): each operand row-major or K32-panel on its own,
// optional second output (pre-activation / act'(pre) / the pre-LayerNorm rows), activation-gradient epilogue, dropout, full-row LayerNorm.
extern "C" int mh_gemm_desc_launch(const mh_gemm_desc* d, mh_stream_t stream) {
  MH_CHECK_ARG(d && d->A && d->W && d->out, "gemm_desc: null pointer");
  MH_CHECK_ARG(d->M > 0 && d->N > 0 && d->K > 0 && d->K % B2K == 0, "gemm_desc: bad problem M=%lld N=%d K=%d", (long long)d->M, d->N, d->K);
  MH_CHECK_ARG(d->act >= MH_ACT_NONE && d->act <= MH_ACT_SILU, "gemm_desc: unknown activation %d", d->act);
  MH_CHECK_ARG(!(d->o_panel && d->out_f32), "gemm_desc: fp32 output is row-major only");
  MH_CHECK_ARG(g_variant >= 2, "gemm_desc: needs the big-tile bf16 kernel");
  GemmArgs g{};
  g.A = d->A; g.lda = d->lda; g.a_panel = d->a_panel; g.W = d->W; g.ldw = d->ldw; g.w_panel = d->w_panel; g.bias = d->bias;
  g.residual = d->residual; g.ldr = d->residual ? d->ldr : 8; g.r_panel = d->residual ? d->r_panel : 0;
  g.out = d->out; g.ldo = d->ldo; g.o_panel = d->o_panel; g.out_f32 = d->out_f32;
  g.pre_out = d->pre_out; g.ldp = d->ldp; g.p_panel = d->p_panel; g.pre_kind = d->pre_kind;
  g.M = d->M; g.N = d->N; g.K = d->K; g.act = d->act; g.act_grad = d->act_grad;
  int rc = mh_drop_args(d->drop, &g.drop);
  if (rc) return rc;
  MH_CHECK_ARG((g.a_panel || g.lda % 8 == 0) && (g.w_panel || g.ldw % 8 == 0) && big_tile_ok(g), "gemm_desc: leading dimensions must be multiples of 8");
  if (d->ln_gamma) {
    MH_CHECK_ARG(d->ln_beta && d->bias && d->residual && d->pre_out, "gemm_desc: the LayerNorm epilogue needs bias, residual, beta and pre_out");
    MH_CHECK_ARG(d->N == 512 && d->act == MH_ACT_NONE && !d->act_grad && !d->out_f32, "gemm_desc: the dropout + LayerNorm epilogue is built for N = 512");
    MH_CHECK_ARG(d->p_panel || (d->ldp ? d->ldp : d->ldo) % 8 == 0, "gemm_desc: ldp must be a multiple of 8");
    g.ln_gamma = d->ln_gamma; g.ln_beta = d->ln_beta; g.ln_eps = d->ln_eps;
    return launch_big<CfgRowPP, 3>(g, (hipStream_t)stream, 1);
  }
  MH_CHECK_ARG(!d->pre_out || d->act != MH_ACT_NONE, "gemm_desc: pre_out without a LayerNorm needs an activation");
  MH_CHECK_ARG(!d->act_grad || d->residual, "gemm_desc: act_grad reads the stored pre-activation / derivative through `residual`");
  return launch<0>(g, MH_BF16, (hipStream_t)stream);
}

extern "C" int mh_gemm_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw, int64_t strideW,
                               const float* bias, void* out, int64_t ldo, int64_t strideO, int out_f32, int batch, int64_t M,
                               int N, int K, int dtype, mh_stream_t stream) {
  MH_CHECK_ARG(A && W && out, "gemm_batched: null pointer");
  MH_CHECK_ARG(M > 0 && N > 0 && batch > 0, "gemm_batched: empty problem");
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.ldr = 8; g.out = out; g.ldo = ldo; g.out_f32 = out_f32;
  g.M = M; g.N = N; g.K = K; g.act = MH_ACT_NONE; g.sA = strideA; g.sW = strideW; g.sO = strideO;
  return launch<0>(g, dtype, (hipStream_t)stream, batch);
}

extern "C" int mh_gemm_qkv(const void* A, int64_t lda, const void* Wqkv, int64_t ldw, const float* bqkv, void* q,
                           void* k, void* vt, int B, int L, int H, int nh, int dtype, mh_stream_t stream) {
  return mh_gemm_qkv_ex(A, lda, 0, Wqkv, ldw, 0, bqkv, q, k, vt, B, L, H, nh, dtype, stream);
}

namespace { int qkv_impl(const void* A, int64_t lda, int a_panel, const void* Wqkv, int64_t ldw, int w_panel, const float* bqkv,
                         void* q, void* k, void* vt, int B, int L, int H, int nh, int dtype, int vt_perm, mh_stream_t stream,
                         const mh_ln_defer* defer = nullptr, float q_scale = 0.f); }

// mh_gemm_qkv_vtperm (panel operands) whose A rows are raw pre-LayerNorm values (defer->a_stats / c1; bqkv = c2)
extern "C" int mh_gemm_qkv_vtperm_defer(const void* A, int64_t lda, const void* Wqkv, int64_t ldw, const float* c2, void* q, void* k,
                                        void* vt_perm, int B, int L, int H, int nh, const mh_ln_defer* defer, mh_stream_t stream) {
  MH_CHECK_ARG(L % 16 == 0, "gemm_qkv_vtperm_defer: seq_len %d must be a multiple of 16", L);
  MH_CHECK_ARG(g_variant >= 2 && defer && defer->a_stats, "gemm_qkv_vtperm_defer: needs the big-tile bf16 kernel and a_stats");
  return qkv_impl(A, lda, 1, Wqkv, ldw, 1, c2, q, k, vt_perm, B, L, H, nh, MH_BF16, 1, stream, defer);
}

extern "C" int mh_gemm_qkv_ex(const void* A, int64_t lda, int a_panel, const void* Wqkv, int64_t ldw, int w_panel,
                              const float* bqkv, void* q, void* k, void* vt, int B, int L, int H, int nh, int dtype,
                              mh_stream_t stream) {
  return qkv_impl(A, lda, a_panel, Wqkv, ldw, w_panel, bqkv, q, k, vt, B, L, H, nh, dtype, 0, stream);
}

extern "C" int mh_gemm_qkv_vtperm(const void* A, int64_t lda, int a_panel, const void* Wqkv, int64_t ldw, int w_panel,
                                  const float* bqkv, void* q, void* k, void* vt_perm, int B, int L, int H, int nh,
                                  mh_stream_t stream) {
  MH_CHECK_ARG(L % 16 == 0, "gemm_qkv_vtperm: seq_len %d must be a multiple of 16", L);
  MH_CHECK_ARG(g_variant >= 2, "gemm_qkv_vtperm: needs the big-tile bf16 kernel");
  return qkv_impl(A, lda, a_panel, Wqkv, ldw, w_panel, bqkv, q, k, vt_perm, B, L, H, nh, MH_BF16, 1, stream);
}
// the same with the queries stored as (x Wq^T + bq) * q_scale (one rounding, from the fp32 accumulator): q_scale = softmax scale x log2(e)
// is what mh_attention_stream_fwd_prescaled expects; defer may be NULL
extern "C" int mh_gemm_qkv_vtperm_qs(const void* A, int64_t lda, const void* Wqkv, int64_t ldw, const float* bqkv, void* q, void* k,
                                     void* vt_perm, int B, int L, int H, int nh, float q_scale, const mh_ln_defer* defer, mh_stream_t stream) {
  MH_CHECK_ARG(L % 16 == 0, "gemm_qkv_vtperm_qs: seq_len %d must be a multiple of 16", L);
  MH_CHECK_ARG(g_variant >= 2 && q_scale > 0.f, "gemm_qkv_vtperm_qs: needs the big-tile bf16 kernel and a positive scale");
  MH_CHECK_ARG(!defer || defer->a_stats, "gemm_qkv_vtperm_qs: a deferred LayerNorm descriptor needs a_stats");
  return qkv_impl(A, lda, 1, Wqkv, ldw, 1, bqkv, q, k, vt_perm, B, L, H, nh, MH_BF16, 1, stream, defer, q_scale);
}

namespace {
int qkv_impl(const void* A, int64_t lda, int a_panel, const void* Wqkv, int64_t ldw, int w_panel, const float* bqkv,
             void* q, void* k, void* vt, int B, int L, int H, int nh, int dtype, int vt_perm, mh_stream_t stream,
             const mh_ln_defer* defer, float q_scale) {
  MH_CHECK_ARG(A && Wqkv && bqkv && q && k && vt, "gemm_qkv: null pointer");
  MH_CHECK_ARG(H % 64 == 0, "gemm_qkv: hidden size %d must be a multiple of 64", H);
  MH_CHECK_ARG(nh > 0 && H % nh == 0 && (H / nh) % 8 == 0, "gemm_qkv: head dim must be a multiple of 8");
  MH_CHECK_ARG(L % 8 == 0, "gemm_qkv: seq_len %d must be a multiple of 8", L);
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = Wqkv; g.ldw = ldw; g.bias = bqkv; g.ldr = 8; g.ldo = 8;
  g.M = (int64_t)B * L; g.N = 3 * H; g.K = H;
  g.a_panel = a_panel; g.w_panel = w_panel;
  g.q = q; g.k = k; g.vt = vt; g.L = L; g.H = H; g.nh = nh; g.dh = H / nh;
  g.vt_perm = vt_perm;
  g.q_scale = q_scale;
  int rcd = fill_defer(defer, g, "gemm_qkv");
  if (rcd) return rcd;
  MH_CHECK_ARG(!vt_perm || (big_tile_ok(g) && H % 64 == 0), "gemm_qkv_vtperm: shape not served by the big-tile kernel");
  return launch<1>(g, dtype, (hipStream_t)stream);
}
}  // namespace


// ---------------------------------------------------------------- nearest-embedding rounding on the fp32 MFMA
namespace {

#pragma clang fp contract(off)
__global__ void row_sqnorm_f32_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t rows, int E) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane; c < E; c += 64) {
    const float v = x[row * ldx + c];
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

__global__ void argbest_reduce_kernel(const float* __restrict__ pbest, const int32_t* __restrict__ pidx, int nslots,
                                      int32_t* __restrict__ idx_out, int64_t rows) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int s = 0; s < nslots; ++s) {   // slots are in increasing column order: strict > keeps the first index
    const float v = pbest[row * nslots + s];
    const int i = pidx[row * nslots + s];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
  idx_out[row] = bi == 0x7fffffff ? 0 : bi;
}

}  // namespace

extern "C" size_t mh_round_workspace_bytes(int64_t n_tokens, int E, int V) {
  const int64_t nslots = 2 * ((V + BN - 1) / BN);
  const int64_t Ep = (E + 15) / 16 * 16;
  size_t b = (size_t)n_tokens * 4;                         // |x_n|^2
  b += (size_t)n_tokens * nslots * 8;                      // partial (score, index)
  if (Ep != E) b += (size_t)n_tokens * Ep * 4;             // zero-padded copy of x
  return b + 1024;
}

// table_pad: [V, E_pad16] fp32 (rows zero-padded to a multiple of 16 columns; == table when E % 16 == 0)
extern "C" int mh_round_to_embedding_mfma(const float* x, const float* table_pad, const float* table_norm, int32_t* idx,
                                          int64_t n_tokens, int E, int V, void* workspace, size_t workspace_bytes,
                                          mh_stream_t stream) {
  MH_CHECK_ARG(x && table_pad && table_norm && idx && workspace, "round_to_embedding_mfma: null pointer");
  MH_CHECK_ARG(n_tokens > 0 && E > 0 && V > 0, "round_to_embedding_mfma: bad shape");
  MH_CHECK_ARG(workspace_bytes >= mh_round_workspace_bytes(n_tokens, E, V), "round_to_embedding_mfma: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nslots = 2 * ceil_div(V, BN);
  const int Ep = (E + 15) / 16 * 16;
  char* ws = (char*)workspace;
  float* rown = (float*)ws; ws += ((size_t)n_tokens * 4 + 255) & ~(size_t)255;
  float* pbest = (float*)ws; ws += ((size_t)n_tokens * nslots * 4 + 255) & ~(size_t)255;
  int32_t* pidx = (int32_t*)ws; ws += ((size_t)n_tokens * nslots * 4 + 255) & ~(size_t)255;
  const float* xa = x;
  int64_t lda = E;
  if (Ep != E) {
    float* xp = (float*)ws;
    int rc = mh_cast_pad(x, E, xp, Ep, n_tokens, E, n_tokens, MH_F32, stream);
    if (rc) return rc;
    xa = xp; lda = Ep;
  }
  MH_LAUNCH(row_sqnorm_f32_kernel, dim3((unsigned)((n_tokens + 3) / 4)), dim3(256), 0, s, x, (int64_t)E, rown, n_tokens, E);
  MH_CHECK_LAUNCH();
  GemmArgs g{};
  g.A = xa; g.lda = lda; g.W = table_pad; g.ldw = Ep; g.ldr = 8; g.ldo = 8;
  g.M = n_tokens; g.N = V; g.K = Ep;
  g.aux = table_norm; g.rown = rown; g.pbest = pbest; g.pidx = pidx; g.nslots = nslots;
  int rc = launch<2>(g, MH_F32, s);
  if (rc) return rc;
  MH_LAUNCH(argbest_reduce_kernel, dim3((unsigned)((n_tokens + 255) / 256)), dim3(256), 0, s, pbest, pidx, nslots, idx, n_tokens);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// The score GEMM of mh_round_to_embedding_mfma alone: |x_n|^2 comes from the caller (the fused down-projection writes it beside its
// rows, csrc/headtail.hip) and the per-slot winners stay in pbest / pidx [n_tokens][mh_round_slots(V)] for mh_step_epilogue_slots to
// fold - two launches less per batch slice and step.  E % 16 == 0 (no padded copy here).
extern "C" int mh_round_slots(int V) { return 2 * ceil_div(V, BN); }
extern "C" int mh_round_scores(const float* x, const float* x_sqnorm, const float* table_pad, const float* table_norm, float* pbest,
                               int32_t* pidx, int64_t n_tokens, int E, int V, mh_stream_t stream) {
  MH_CHECK_ARG(x && x_sqnorm && table_pad && table_norm && pbest && pidx && n_tokens > 0 && V > 0, "round_scores: bad arguments");
  MH_CHECK_ARG(E > 0 && E % 16 == 0, "round_scores: E = %d must be a multiple of 16", E);
  GemmArgs g{};
  g.A = x; g.lda = E; g.W = table_pad; g.ldw = E; g.ldr = 8; g.ldo = 8;
  g.M = n_tokens; g.N = V; g.K = E;
  g.aux = table_norm; g.rown = x_sqnorm; g.pbest = pbest; g.pidx = pidx; g.nslots = mh_round_slots(V);
  return launch<2>(g, MH_F32, (hipStream_t)stream);
}

