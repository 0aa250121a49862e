// Weight-gradient GEMM ("TN"): dW[m][n] = sum_k A[k][m] * B[k][n] with BOTH operands stored k-major (A = dY [tokens, out
// features], B = X [tokens, in features], exactly as the forward wrote them) - no transposed copies.  The reduction runs over
// the tokens, the output is tiny, so the token range is cut into `splits` slices (grid.y) that write fp32 partials
// [splits][M][N] for mh_sum_slices.  Tile 256 (m) x 128 (n), 4 waves of 128 x 64, K-step 32 tokens, 3-stage LDS-DMA ring
// as in gemm_big_kernel.  The LDS image keeps the k-major rows ([32 k][256 m] and [32 k][128 n]); MFMA fragments
// (8 consecutive k of one m / n per lane) come out of it through the transposing read ds_read_b64_tr_b16, two per fragment.
// 16-byte chunk c of row k is stored at c ^ f(k), f(k) = 2 ((k & 3) | ((k >> 3 & 1) << 2)) (applied on the DMA source
// address): the 8 rows a 32-lane half reads in one instruction then fall on 8 different 32-byte bank slots.
#include "gemm_args.h"

using namespace mhgemm;

namespace {

struct TnArgs {
  const bf16* A; int64_t lda;   // [K, lda], columns = m
  const bf16* B; int64_t ldb;   // [K, ldb], columns = n
  float* out;                   // [splits][slice]: M x N products, then (CS) the M column sums of A
  int M, N;
  int64_t Ksteps;               // K steps (32 tokens each) in all; slice s of `splits` runs steps [s Ksteps / splits, (s + 1) Ksteps / splits)
  int64_t slice;                // floats per split slice: M N (+ M)
  int splits, tiles;            // grid = tiles x splits blocks, one-dimensional (see the block mapping in the kernel)
};

typedef __attribute__((ext_vector_type(4))) short s16x4;

__device__ __forceinline__ int tn_f(int row) { return ((row & 3) | (((row >> 3) & 1) << 2)) << 1; }

// CS > 0: the kernel also writes the column sums of A over its token slice (the bias gradient of the same linear: A = dY) behind
// the M x N products of the slice.  They come out of the matrix pipe - one more MFMA against an all-ones operand gives sum_k A[k][m]
// in every row of the product - and the work is dealt out over the blocks and waves that share a 256-column panel of A: CS = number
// of (n-tile, wave column) workers taking part (2, 4 or 8), worker w sums the 16-column tiles i with i % CS == w.
// WN = wave columns of 64 output columns each: 2 -> the 256 x 128 tile on 4 waves, two blocks per CU; 4 -> a 256 x 256 tile on 8 waves,
// one block per CU - the same waves per SIMD and the same wave tile, but HALF the blocks for the same chip occupancy: the fp32
// partials of a launch (one tile per block: blocks x 128 KiB, whatever the shape) and their fold by mh_sum_slices halve, and both
// operand panels are read once per 256 x 256 outputs.
// PANEL (round 6): both operands as K32 panels [cols / 32][ld rows][32] - the layout every GEMM operand of the training step has since the
// forward and input-gradient GEMMs moved onto the sampler's panel tiles.  A stage keeps the panels apart ([panel][32 k][64 B]: one DMA piece =
// 16 consecutive tokens of one panel = 1 KiB of contiguous memory), the transposing reads address 64-byte rows, and the 32-byte halves of a row
// swap for k rows 8 - 15 / 24 - 31 (on the DMA source address) so that the 8 rows of a 32-lane half fall on 8 different 32-byte bank slots.
template <int CS, int WN = 2, bool PANEL = false>
__global__ __launch_bounds__(128 * WN, WN == 2 ? 2 : 1) void gemm_tn_kernel(const TnArgs g) {
  constexpr int BMt = 256, BNt = 64 * WN, NWt = 2 * WN, NSTt = 3, ASTAGE = 32 * BMt * 2, BSTAGE = 32 * BNt * 2, STAGEt = ASTAGE + BSTAGE;
  constexpr int TIt = 8, TJt = 4;
  constexpr int PAt = 16 / NWt, PBt = (BSTAGE / 1024) / NWt;     // 1-KiB DMA pieces per wave and stage: A 4 / 2, B 2
  constexpr int CPRB = BNt / 8, RPPB = 64 / CPRB;                // B: 16-byte chunks per k-row, k-rows per piece
  __shared__ __attribute__((aligned(16))) char smem[NSTt * STAGEt];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (g.N + BNt - 1) / BNt;
  // XCD-aware block mapping (round 6): the blocks of ONE token slice share its operand panels (every m-tile's A panels are read by all
  // n-tiles and vice versa), and workgroups go to the 8 XCDs round-robin - dealt out as (tile, slice) = (blockIdx.x, blockIdx.y) the 16 tiles
  // of a slice landed on all 8 L2s and every panel was fetched from HBM up to 8 times (rocprofv3 FETCH_SIZE: 313 MB per launch against
  // 167 MB of operands).  mh_xcd_remap gives each XCD a contiguous run of (slice, tile) pairs, i.e. whole slices.
  const int vb = mh_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int slice_i = vb / g.tiles, tile_i = vb % g.tiles;
  const int m0 = (tile_i / tiles_n) * BMt, n0 = (tile_i % tiles_n) * BNt;
  // (uneven slices: the split count is chosen to fill the chip - 21 slices of a 12-tile output on 256 CUs - not to divide the K steps)
  const int64_t ks0 = (int64_t)slice_i * g.Ksteps / g.splits, ks1 = (int64_t)(slice_i + 1) * g.Ksteps / g.splits;
  const int64_t k_begin = ks0 * 32;
  const int nk = (int)(ks1 - ks0);
  const int fr = lane & 15, fg = lane >> 4;

  // DMA: A stage = 16 pieces of (2 k-rows x 512 B); B stage = pieces of (RPPB k-rows x BNt * 2 B)
  const bf16* srcA[PAt];
  const bf16* srcB[PBt];
  if constexpr (PANEL) {
    // piece = (panel of the tile, half of the stage's 32 tokens); lane i lands at token i / 4, physical chunk i % 4
    const int rl = lane >> 2, pc = lane & 3;
#pragma unroll
    for (int j = 0; j < PAt; ++j) {
      const int piece = wave * PAt + j, row = (piece & 1) * 16 + rl, lc = pc ^ (((row >> 3) & 1) << 1);
      int pn = (m0 >> 5) + (piece >> 1);
      if (pn > (g.M >> 5) - 1) pn = (g.M >> 5) - 1;         // M % 32 == 0: clamp whole panels (results beyond M are not stored)
      srcA[j] = g.A + ((int64_t)pn * g.lda + k_begin + row) * 32 + lc * 8;
    }
#pragma unroll
    for (int j = 0; j < PBt; ++j) {
      const int piece = wave * PBt + j, row = (piece & 1) * 16 + rl, lc = pc ^ (((row >> 3) & 1) << 1);
      int pn = (n0 >> 5) + (piece >> 1);
      if (pn > (g.N >> 5) - 1) pn = (g.N >> 5) - 1;
      srcB[j] = g.B + ((int64_t)pn * g.ldb + k_begin + row) * 32 + lc * 8;
    }
  } else {
#pragma unroll
  for (int j = 0; j < PAt; ++j) {
    const int piece = wave * PAt + j, row = piece * 2 + (lane >> 5), pc = lane & 31;
    int col = m0 + ((pc ^ tn_f(row)) << 3);
    if (col > g.M - 8) col = g.M - 8;                       // M % 8 == 0: clamp whole chunks (results beyond M are not stored)
    srcA[j] = g.A + (k_begin + row) * g.lda + col;
  }
#pragma unroll
  for (int j = 0; j < PBt; ++j) {
    const int piece = wave * PBt + j, row = piece * RPPB + lane / CPRB, pc = lane % CPRB;
    int col = n0 + ((pc ^ tn_f(row)) << 3);
    if (col > g.N - 8) col = g.N - 8;
    srcB[j] = g.B + (k_begin + row) * g.ldb + col;
  }
  }
  const int64_t kadvA = PANEL ? 32 * 32 : 32 * g.lda, kadvB = PANEL ? 32 * 32 : 32 * g.ldb;   // elements per K step (32 tokens)
  auto issue = [&](int kt) {
    char* base = smem + (kt % NSTt) * STAGEt;
#pragma unroll
    for (int j = 0; j < PAt; ++j)
      mh_glds16(srcA[j] + (int64_t)kt * kadvA, base + (wave * PAt + j) * 1024);
#pragma unroll
    for (int j = 0; j < PBt; ++j)
      mh_glds16(srcB[j] + (int64_t)kt * kadvB, base + ASTAGE + (wave * PBt + j) * 1024);
  };
  // transposing reads: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a (4 k) x (16 columns) block and
  // receives column (lane & 15) of the 4 rows.  Group = k-group fg: rows 8 fg + 4 half + q.
  const int q = (lane & 15) >> 2, p = lane & 3;
  int offA[2], offB[2];                                    // byte offsets inside a stage for half = 0 / 1, column tile 0
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = 8 * fg + 4 * half + q;
    const int f = tn_f(row);
    if constexpr (PANEL) {   // (row start + the lane's 8 bytes inside a 32-byte half; frag_half adds the panel and the half)
      offA[half] = row * 64 + ((p >> 1) << 4) + ((p & 1) << 3);
      offB[half] = ASTAGE + offA[half];
      continue;
    }
    // column 4p of a 16-column tile starting at a multiple of 16: chunk (tile*2 + (p >> 1)) ^ f, byte (p & 1) * 8
    offA[half] = row * (BMt * 2) + ((((p >> 1)) ^ f) << 4) + ((p & 1) << 3);
    offB[half] = ASTAGE + row * (BNt * 2) + ((((p >> 1)) ^ f) << 4) + ((p & 1) << 3);
  }
  // The transposing reads are issued as inline asm: behind the intrinsic form hipcc puts `s_waitcnt vmcnt(0)` in front of the first
  // read of every K-step (it cannot tell that the read does not alias the LDS-DMA stage it has just queued), which turns the
  // three-stage ring into a synchronous copy.  The asm form hides the reads from that analysis; their results are only touched
  // after the explicit lgkmcnt(0) below, which names them as operands so that nothing that uses them can move above it.
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  auto frag_half = [&](unsigned stage_off, const int (&off)[2], int tile16, int half) -> s16x4 {
    // tile16 = index of the 16-column tile: its two chunks are 2*tile16, 2*tile16 + 1, XOR-ed with the row's swizzle f
    const int row = 8 * fg + 4 * half + q;
    unsigned addr;
    if constexpr (PANEL) {   // panel tile16 / 2 of the operand's stage, 64-byte rows, 32-byte half (tile16 & 1) ^ (row bit 3)
      addr = lds0 + stage_off + off[half] + (tile16 >> 1) * 2048 + (((tile16 & 1) ^ ((row >> 3) & 1)) << 5);
    } else {
    const int f = tn_f(row);
    const int base = off[half] - (((p >> 1) ^ f) << 4);          // row start (+ byte-in-chunk)
    addr = lds0 + stage_off + base + ((((tile16 << 1) + (p >> 1)) ^ f) << 4);
    }
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
    return v;
  };
  auto join = [](const s16x4& lo, const s16x4& hi) -> bf16x8 {
    bf16x8 r;
    __builtin_memcpy(&r, &lo, 8);
    __builtin_memcpy(reinterpret_cast<char*>(&r) + 8, &hi, 8);
    return r;
  };

  f32x4 acc[TIt][TJt];
#pragma unroll
  for (int i = 0; i < TIt; ++i)
#pragma unroll
    for (int j = 0; j < TJt; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int NCS = TIt / (CS > 0 ? CS : TIt);            // column-sum tiles per worker
  f32x4 accs[NCS];
#pragma unroll
  for (int c = 0; c < NCS; ++c) accs[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int worker = (tile_i % tiles_n) * WN + wn;  // (wave-uniform)
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (bf16)1.0f;

  const int npro = nk < NSTt - 1 ? nk : NSTt - 1;
  for (int st = 0; st < npro; ++st) issue(st);
  for (int kt = 0; kt < nk; ++kt) {
    const int younger = nk - 1 - kt < NSTt - 2 ? nk - 1 - kt : NSTt - 2;
    mh_wait_stages<PAt + PBt>(younger);
    __builtin_amdgcn_s_barrier();
    if (kt + NSTt - 1 < nk) issue(kt + NSTt - 1);
    const unsigned stage = (unsigned)((kt % NSTt) * STAGEt);
    s16x4 ah[TIt][2], bh[TJt][2];
#pragma unroll
    for (int j = 0; j < TJt; ++j) { bh[j][0] = frag_half(stage, offB, wn * 4 + j, 0); bh[j][1] = frag_half(stage, offB, wn * 4 + j, 1); }
#pragma unroll
    for (int i = 0; i < TIt; ++i) { ah[i][0] = frag_half(stage, offA, wm * 8 + i, 0); ah[i][1] = frag_half(stage, offA, wm * 8 + i, 1); }
    static_assert(TIt == 8 && TJt == 4, "the wait below names the 24 fragment halves");
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(ah[0][0]), "+v"(ah[0][1]), "+v"(ah[1][0]), "+v"(ah[1][1]), "+v"(ah[2][0]), "+v"(ah[2][1]), "+v"(ah[3][0]), "+v"(ah[3][1]),
                   "+v"(ah[4][0]), "+v"(ah[4][1]), "+v"(ah[5][0]), "+v"(ah[5][1]), "+v"(ah[6][0]), "+v"(ah[6][1]), "+v"(ah[7][0]), "+v"(ah[7][1]),
                   "+v"(bh[0][0]), "+v"(bh[0][1]), "+v"(bh[1][0]), "+v"(bh[1][1]), "+v"(bh[2][0]), "+v"(bh[2][1]), "+v"(bh[3][0]), "+v"(bh[3][1]));
    bf16x8 a[TIt], b[TJt];
#pragma unroll
    for (int j = 0; j < TJt; ++j) b[j] = join(bh[j][0], bh[j][1]);
#pragma unroll
    for (int i = 0; i < TIt; ++i) a[i] = join(ah[i][0], ah[i][1]);
#pragma unroll
    for (int i = 0; i < TIt; ++i)
#pragma unroll
      for (int j = 0; j < TJt; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);   // D'[n][m]
    if constexpr (CS > 0) {
      if (worker < CS) {
#pragma unroll
        for (int c = 0; c < NCS; ++c) {
          bf16x8 ac = a[c * CS];
#pragma unroll
          for (int w = 1; w < CS; ++w) if (worker == w) ac = a[c * CS + w];
          accs[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, ac, accs[c], 0, 0, 0);
        }
      }
    }
    mh_wait_lgkmcnt0();
  }
  // D' tile (rows n, cols m): lane holds m = fr, n = 4 fg + r -> 4 consecutive n of one m: one 16-byte store
  float* outp = g.out + (int64_t)slice_i * g.slice;
  if constexpr (CS > 0) {
    if (worker < CS && fg == 0) {                           // every row of the ones-product holds the sums: take row 0 (lanes 0..15)
#pragma unroll
      for (int c = 0; c < NCS; ++c) {
        const int m = m0 + wm * 128 + 16 * (c * CS + worker) + fr;
        if (m < g.M) outp[(int64_t)g.M * g.N + m] = accs[c][0];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TIt; ++i) {
    const int m = m0 + wm * 128 + 16 * i + fr;
    if (m < g.M) {
#pragma unroll
      for (int j = 0; j < TJt; ++j) {
        const int n = n0 + wn * 64 + 16 * j + 4 * fg;
        if (n < g.N) *reinterpret_cast<f32x4*>(outp + (int64_t)m * g.N + n) = acc[i][j];
      }
    }
  }
}

}  // namespace

namespace { MH_KNOB(int, g_dw_blocks, 512); MH_KNOB(int, g_dw_wide, 1); }
// blocks a weight-gradient launch aims for when it cuts the token range (A/B knob; 512 = two 4-wave blocks per CU; the 256 x 256
// tile's 8-wave blocks count double)
#ifdef MH_ABLATE
extern "C" int mh_gemm_dw_set_blocks(int blocks) {
  g_dw_blocks = blocks < 1 ? 1 : blocks;
  return MH_OK;
}
#endif
// A/B: 0 = always the 256 x 128 tile (round 2), 1 = the 256 x 256 tile where N is a multiple of 256
#ifdef MH_ABLATE
extern "C" int mh_gemm_dw_set_wide(int on) {
  g_dw_wide = on ? 1 : 0;
  return MH_OK;
}
#endif
namespace { bool dw_wide(int N) { return g_dw_wide && N % 256 == 0; } }

extern "C" int mh_gemm_dw_splits(int64_t K, int M, int N) {
  const bool wide = dw_wide(N);
  const int tiles = ceil_div(M, 256) * ceil_div(N, wide ? 256 : 128);
  const int target = wide ? (g_dw_blocks + 1) / 2 : g_dw_blocks;
  // as many slices as keep every block slot of the chip busy ONCE (round 6: any count - the slices may differ by one K step; rounds 2 - 5
  // doubled the count until it reached the target, which ran the [1536 x 512] gradient's 12 tiles as 384 blocks = 1.5 rounds on 256 CUs),
  // at most 64 and at least 16 K steps (512 tokens) per slice
  int64_t S = target / tiles;
  const int64_t ksteps = K / 32;
  if (S > ksteps / 16) S = ksteps / 16;
  if (S > 64) S = 64;
  if (S < 1) S = 1;
  return (int)S;
}

// dW = A^T B for k-major bf16 operands: out_partials [splits][M][N] fp32 (splits = mh_gemm_dw_splits(K, M, N); fold with
// mh_sum_slices).  M, N multiples of 8, lda / ldb multiples of 8, K a multiple of 32 * splits.

extern "C" int mh_gemm_dw(const void* A, int64_t lda, const void* B, int64_t ldb, float* out_partials, int splits, int64_t K, int M,
                          int N, mh_stream_t stream) {
  return mh_gemm_dw_bias(A, lda, B, ldb, out_partials, splits, K, M, N, 0, stream);
}

// with_colsum != 0: every split slice is M N + M floats - the products, then the column sums of A over the slice's tokens (A = dY:
// the bias gradient of the linear whose weight gradient this is); one mh_sum_slices over M N + M elements folds both.
extern "C" int mh_gemm_dw_bias(const void* A, int64_t lda, const void* B, int64_t ldb, float* out_partials, int splits, int64_t K, int M,
                               int N, int with_colsum, mh_stream_t stream) {
  return mh_gemm_dw_bias_ex(A, lda, B, ldb, 0, out_partials, splits, K, M, N, with_colsum, stream);
}

// panel != 0: both operands as K32 panels [cols / 32][ld rows][32] (lda / ldb = rows of the panel buffers, M and N multiples of 32)
extern "C" int mh_gemm_dw_bias_ex(const void* A, int64_t lda, const void* B, int64_t ldb, int panel, float* out_partials, int splits, int64_t K,
                                  int M, int N, int with_colsum, mh_stream_t stream) {
  MH_CHECK_ARG(A && B && out_partials, "gemm_dw: null pointer");
  MH_CHECK_ARG(!panel || (M % 32 == 0 && N % 32 == 0 && lda >= K && ldb >= K), "gemm_dw: panel operands need M, N multiples of 32 and ld >= K rows");
  MH_CHECK_ARG(M > 0 && N > 0 && M % 8 == 0 && N % 4 == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0, "gemm_dw: M, N, lda, ldb must be multiples of 8");
  MH_CHECK_ARG(splits >= 1 && splits <= 65535 && K > 0 && K % 32 == 0 && splits <= K / 32, "gemm_dw: K=%lld must be a multiple of 32 with at least one K step per split", (long long)K);
  const bool wide = dw_wide(N);
  const int tiles_n = ceil_div(N, wide ? 256 : 128);
  const int tiles = ceil_div(M, 256) * tiles_n;
  MH_CHECK_ARG((int64_t)tiles * splits < (1ll << 31), "gemm_dw: grid too large");
  TnArgs g{(const bf16*)A, lda, (const bf16*)B, ldb, out_partials, M, N, K / 32, (int64_t)M * N + (with_colsum ? M : 0), splits, tiles};
  const dim3 grid((unsigned)(tiles * splits));
  mh_prof_note("gemm_dw M=%d N=%d K=%lld splits=%d colsum=%d tile=256x%d", M, N, (long long)K, splits, with_colsum != 0, wide ? 256 : 128);
  hipStream_t st = (hipStream_t)stream;
  if (panel && wide) {
    if (!with_colsum) MH_LAUNCH((gemm_tn_kernel<0, 4, true>), grid, dim3(512), 0, st, g);
    else if (tiles_n >= 2) MH_LAUNCH((gemm_tn_kernel<8, 4, true>), grid, dim3(512), 0, st, g);
    else MH_LAUNCH((gemm_tn_kernel<4, 4, true>), grid, dim3(512), 0, st, g);
  }
  else if (panel) {
    if (!with_colsum) MH_LAUNCH((gemm_tn_kernel<0, 2, true>), grid, dim3(256), 0, st, g);
    else if (tiles_n >= 4) MH_LAUNCH((gemm_tn_kernel<8, 2, true>), grid, dim3(256), 0, st, g);
    else if (tiles_n >= 2) MH_LAUNCH((gemm_tn_kernel<4, 2, true>), grid, dim3(256), 0, st, g);
    else MH_LAUNCH((gemm_tn_kernel<2, 2, true>), grid, dim3(256), 0, st, g);
  }
  else if (wide) {   // column-sum workers = n-tiles x 4 wave columns
    if (!with_colsum) MH_LAUNCH((gemm_tn_kernel<0, 4>), grid, dim3(512), 0, st, g);
    else if (tiles_n >= 2) MH_LAUNCH((gemm_tn_kernel<8, 4>), grid, dim3(512), 0, st, g);
    else MH_LAUNCH((gemm_tn_kernel<4, 4>), grid, dim3(512), 0, st, g);
  }
  else if (!with_colsum) MH_LAUNCH(gemm_tn_kernel<0>, grid, dim3(256), 0, st, g);
  else if (tiles_n >= 4) MH_LAUNCH(gemm_tn_kernel<8>, grid, dim3(256), 0, st, g);
  else if (tiles_n >= 2) MH_LAUNCH(gemm_tn_kernel<4>, grid, dim3(256), 0, st, g);
  else MH_LAUNCH(gemm_tn_kernel<2>, grid, dim3(256), 0, st, g);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
