// Evaluation of sampled batches on the device (include/musehip_eval.h): the fused MSIM 1-nearest-neighbour search.
// Reference: MuseDiffusion/metric.py:96-105 (three Gram matrices, their element-wise product, fill_diagonal_(0), argmax over each row).
// Here the similarity of a (query, key) pair lives in one register and only the running (value, index) pair of each query row is kept:
// the N x N matrix is never written unless the caller asks for it.
//
// Form: 256 threads = 4 waves per block.  Keys go through LDS in tiles of KT rows (rows padded to 60 floats: 30 KiB a tile); the tile
// after the one in work is already on its way into registers (28 floats a thread), so no global latency stands between two tiles.
// A wave is SL slices of 64 / SL lanes: lane l holds query row (block's first) + l % (64 / SL) in 56 registers and walks slice
// l / (64 / SL) of its wave's quarter of every tile, so all lanes of a slice read the same key row at the same time (one LDS address
// per slice: a broadcast; the 60-float row stride puts the slices of one ds_read_b128 lane group on different banks).  SL = 1, 2, 4
// is chosen per launch so that a small query set still spreads over the chip: 64, 32 or 16 query rows per block.  A lane meets
// its keys in ascending index, so "strictly better" keeps the lowest index among equals; the 4 SL partial pairs of a query row are
// combined in LDS by the full rule.  What a pair (i, j) computes is msim_pair() whatever the geometry.  FP32 VALU and LDS-read bound
// (56 fused multiply-adds and 14 ds_read_b128 per slice and key), no MFMA shape: a pair's operation order is pinned.
#include "common.h"
#include "msim_pair.h"

#include "../../include/musehip_eval.h"

namespace {

constexpr int TB = 256;
constexpr int NW = TB / 64;         // waves per block
constexpr int KT = 128;             // key rows per tile == mhe_nearest_key_tile()
constexpr int KW = KT / NW;         // key rows per wave and tile
using msim::D;
constexpr int LD = 60;              // LDS row stride in floats: 16-byte rows, and (KW / 4) * LD = 480 = 32 mod 64 banks
constexpr int PRE = KT * D / TB;    // floats of a tile each thread moves
static_assert(KT * LD * sizeof(float) <= 32 * 1024, "a key tile stays within 32 KiB of LDS");
static_assert(KT * D % TB == 0 && KT <= TB && LD % 4 == 0 && LD >= D, "staging layout");

// the similarity of one pair is msim::msim_pair() (msim_pair.h): the operation order the header states, whatever wave, slice, tile slot
// or grid handles the pair
using msim::msim_pair;

// torch.argmax's order on (value, index) pairs with index -1 = no candidate: does (a, ja) come before (b, jb)?
__device__ __forceinline__ bool pair_wins(float a, int ja, float b, int jb) {
  if (ja < 0) return false;
  if (jb < 0) return true;
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ja < jb);
  return a > b || (a == b && ja < jb);
}

template <int SL>
__global__ __launch_bounds__(TB) void msim_nearest_kernel(const float* __restrict__ q, int nq, const float* __restrict__ k, int nk,
                                                         const int32_t* __restrict__ q_valid, const int32_t* __restrict__ k_valid, int self,
                                                         int32_t* __restrict__ most, float* __restrict__ best, float* __restrict__ sim) {
  constexpr int QW = 64 / SL;       // query rows per block
  constexpr int KS = KW / SL;       // key rows per slice and tile
  __shared__ __attribute__((aligned(16))) float tile[KT * LD];
  __shared__ int32_t tile_valid[KT];
  __shared__ float part_v[NW * SL][QW];
  __shared__ int32_t part_j[NW * SL][QW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = wave * SL + lane / QW;                    // which KS rows of every tile this lane walks
  const int row = blockIdx.x * QW + lane % QW;
  const bool q_in = row < nq;
  const int qrow = q_in ? row : nq - 1;                      // a lane past the end computes on the last row and stores nothing
  const bool q_on = q_in && (q_valid == nullptr || q_valid[qrow] != 0);
  float qv[D];
#pragma unroll
  for (int e = 0; e < D; ++e) qv[e] = q[qrow * D + e];

  // a tile is one contiguous run of the key array: thread t moves its elements t, t + TB, ...
  float pre[PRE];
  int32_t pre_valid = 0;
  auto fetch = [&](int j0) {
    const int n = min(KT, nk - j0) * D;
    const float* __restrict__ src = k + (int64_t)j0 * D;
#pragma unroll
    for (int i = 0; i < PRE; ++i) pre[i] = tid + i * TB < n ? src[tid + i * TB] : 0.0f;
    pre_valid = tid < KT && j0 + tid < nk && (k_valid == nullptr || k_valid[j0 + tid] != 0);
  };
  fetch(0);
  float bv = 0.0f;
  int bj = -1;
  for (int j0 = 0; j0 < nk; j0 += KT) {
#pragma unroll
    for (int i = 0; i < PRE; ++i) {
      const int e = tid + i * TB;
      tile[(e / D) * LD + e % D] = pre[i];
    }
    if (tid < KT) tile_valid[tid] = pre_valid;                // rows past nk, masked keys: 0
    __syncthreads();
    if (j0 + KT < nk) fetch(j0 + KT);                        // in flight while this tile is worked on
#pragma unroll 2
    for (int jj = part * KS; jj < (part + 1) * KS; ++jj) {
      if (!tile_valid[jj]) continue;
      const int j = j0 + jj;
      float s = msim_pair(qv, tile + jj * LD);
      if (self && j == row) s = 0.0f;
      if (sim != nullptr && q_on) sim[(int64_t)row * nk + j] = s;
      // ascending j within this lane: only a strictly better value (or the first NaN) replaces the running pair
      if (bj < 0 || (s != s ? bv == bv : s > bv)) { bv = s; bj = j; }
    }
    __syncthreads();                                        // the tile is free for the next one
  }
  part_v[part][lane % QW] = bv;
  part_j[part][lane % QW] = bj;
  __syncthreads();
  if (tid < QW && q_in) {                                    // tid < QW: lane % QW == tid, this thread's own row
    float v = part_v[0][tid];
    int j = part_j[0][tid];
#pragma unroll
    for (int p = 1; p < NW * SL; ++p) {
      const float vp = part_v[p][tid];
      const int jp = part_j[p][tid];
      if (pair_wins(vp, jp, v, j)) { v = vp; j = jp; }
    }
    if (!q_on || j < 0) { v = 0.0f; j = -1; }
    most[row] = j;
    if (best != nullptr) best[row] = v;
  }
}

}  // namespace

extern "C" int mhe_nearest_key_tile(void) { return KT; }

extern "C" int mhe_msim_nearest(const float* q, int64_t nq, const float* k, int64_t nk, const int32_t* q_valid, const int32_t* k_valid, int self,
                                int32_t* most, float* best, float* sim, mh_stream_t stream) {
  constexpr int64_t kMaxRows = 0x7fffffffLL / D;            // n * 56 is a 32-bit element index in the kernel
  MH_CHECK_ARG(q && k && most, "msim_nearest: q, k and most must not be NULL");
  MH_CHECK_ARG(nq >= 1 && nq <= kMaxRows && nk >= 1 && nk <= kMaxRows, "msim_nearest: nq = %lld, nk = %lld outside 1..%lld", (long long)nq,
               (long long)nk, (long long)kMaxRows);
  MH_CHECK_ARG(self == 0 || self == 1, "msim_nearest: self = %d is neither 0 nor 1", self);
  MH_CHECK_ARG(!self || (q == k && nq == nk && q_valid == k_valid),
               "msim_nearest: self = 1 needs q == k, nq == nk and the same validity pointer");
  // the fewest slices per wave (the most query rows per block: the least LDS traffic per pair) that still give every CU a block
  const int64_t cus = mh_device_cus();
  const int sl = (nq + 63) / 64 >= cus ? 1 : (nq + 31) / 32 >= cus ? 2 : 4;
  const dim3 grid((unsigned)((nq + 64 / sl - 1) / (64 / sl)));
  mh_prof_note("nq=%lld nk=%lld slices=%d self=%d", (long long)nq, (long long)nk, sl, self);
  if (sl == 1)
    MH_LAUNCH(msim_nearest_kernel<1>, grid, dim3(TB), 0, (hipStream_t)stream, q, (int)nq, k, (int)nk, q_valid, k_valid, self, most, best, sim);
  else if (sl == 2)
    MH_LAUNCH(msim_nearest_kernel<2>, grid, dim3(TB), 0, (hipStream_t)stream, q, (int)nq, k, (int)nk, q_valid, k_valid, self, most, best, sim);
  else
    MH_LAUNCH(msim_nearest_kernel<4>, grid, dim3(TB), 0, (hipStream_t)stream, q, (int)nq, k, (int)nk, q_valid, k_valid, self, most, best, sim);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
