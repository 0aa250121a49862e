// Statistics over all pairs of a set under the MSIM similarity (include/musehip_stats.h): per query row the float64 sum of its
// similarities and three counts (finite pairs, NaN pairs, pairs at or above a threshold).  What a generation run says about its own
// output without a ground truth - diversity, duplicates - is a reduction of these; the nearest-neighbour kernel (evaluate.hip) keeps
// a maximum per row and cannot give them, and the N x N matrix is never written here either.
//
// Form: that of msim_nearest_kernel.  256 threads = 4 waves per block; keys go through LDS in tiles of KT rows (rows padded to 60
// floats), beside them the tile's validity and group ids; the tile after the one in work is on its way in registers.  A wave is SL
// slices of 64 / SL lanes: lane l holds query row (block's first) + l % (64 / SL) in 56 registers and walks slice l / (64 / SL) of its
// wave's quarter of every tile, so the lanes of a slice read one LDS address (a broadcast).  SL = 1, 2, 4 from nq, so that a small
// set still spreads over the chip.  A pair's value is msim::msim_pair() (msim_pair.h), the function evaluate.hip calls: the same bits.
// Per lane a float64 sum and three int32 counters; a lane meets its keys in ascending index and the 4 SL partials of a row are added
// in LDS in ascending part order by one thread: the order within a launch is fixed, there is no atomic and no workspace.  The float64
// add rides beside 56 fp32 fused multiply-adds per pair.
#include "common.h"
#include "msim_pair.h"

#include "../../include/musehip_stats.h"

namespace {

constexpr int TB = 256;
constexpr int NW = TB / 64;         // waves per block
constexpr int KT = 128;             // key rows per tile == mhs_pair_key_tile()
constexpr int KW = KT / NW;         // key rows per wave and tile
using msim::D;
constexpr int LD = 60;              // LDS row stride in floats: 16-byte rows, and (KW / 4) * LD = 480 = 32 mod 64 banks
constexpr int PRE = KT * D / TB;    // floats of a tile each thread moves
static_assert(KT * LD * sizeof(float) <= 32 * 1024, "a key tile stays within 32 KiB of LDS");
static_assert(KT * D % TB == 0 && KT <= TB && LD % 4 == 0 && LD >= D, "staging layout");

template <int SL>
__global__ __launch_bounds__(TB) void msim_pair_stats_kernel(const float* __restrict__ q, int nq, const float* __restrict__ k, int nk,
                                                            const int32_t* __restrict__ q_valid, const int32_t* __restrict__ k_valid,
                                                            const int32_t* __restrict__ q_group, const int32_t* __restrict__ k_group, int self,
                                                            float threshold, double* __restrict__ sum, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ nan, int32_t* __restrict__ above) {
  constexpr int QW = 64 / SL;       // query rows per block
  constexpr int KS = KW / SL;       // key rows per slice and tile
  __shared__ __attribute__((aligned(16))) float tile[KT * LD];
  __shared__ int32_t tile_valid[KT];
  __shared__ int32_t tile_group[KT];
  __shared__ double part_sum[NW * SL][QW];
  __shared__ int32_t part_count[NW * SL][QW];
  __shared__ int32_t part_nan[NW * SL][QW];
  __shared__ int32_t part_above[NW * SL][QW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = wave * SL + lane / QW;                    // which KS rows of every tile this lane walks
  const int row = blockIdx.x * QW + lane % QW;
  const bool q_in = row < nq;
  const int qrow = q_in ? row : nq - 1;                      // a lane past the end computes on the last row and stores nothing
  const bool q_on = q_in && (q_valid == nullptr || q_valid[qrow] != 0);
  const int32_t qg = q_group == nullptr ? 0 : q_group[qrow];
  const int skip = self ? row : -1;                          // the diagonal is no pair
  float qv[D];
#pragma unroll
  for (int e = 0; e < D; ++e) qv[e] = q[qrow * D + e];

  // a tile is one contiguous run of the key array: thread t moves its elements t, t + TB, ...
  float pre[PRE];
  int32_t pre_valid = 0, pre_group = 0;
  auto fetch = [&](int j0) {
    const int n = min(KT, nk - j0) * D;
    const float* __restrict__ src = k + (int64_t)j0 * D;
#pragma unroll
    for (int i = 0; i < PRE; ++i) pre[i] = tid + i * TB < n ? src[tid + i * TB] : 0.0f;
    const bool in = tid < KT && j0 + tid < nk;
    pre_valid = in && (k_valid == nullptr || k_valid[j0 + tid] != 0);
    pre_group = in && k_group != nullptr ? k_group[j0 + tid] : 0;
  };
  fetch(0);
  double acc = 0.0;
  int32_t cnt = 0, nans = 0, abv = 0;
  for (int j0 = 0; j0 < nk; j0 += KT) {
#pragma unroll
    for (int i = 0; i < PRE; ++i) {
      const int e = tid + i * TB;
      tile[(e / D) * LD + e % D] = pre[i];
    }
    if (tid < KT) {
      tile_valid[tid] = pre_valid;                           // rows past nk, masked keys: 0
      tile_group[tid] = pre_group;
    }
    __syncthreads();
    if (j0 + KT < nk) fetch(j0 + KT);                        // in flight while this tile is worked on
#pragma unroll 2
    for (int jj = part * KS; jj < (part + 1) * KS; ++jj) {
      if (!tile_valid[jj]) continue;
      const float s = msim::msim_pair(qv, tile + jj * LD);
      // ascending j within this lane; a pair of another group, or the diagonal, leaves every accumulator as it is
      if (tile_group[jj] == qg && j0 + jj != skip) {
        if (s != s) {
          ++nans;
        } else {
          ++cnt;
          acc += (double)s;
          abv += s >= threshold;
        }
      }
    }
    __syncthreads();                                        // the tile is free for the next one
  }
  part_sum[part][lane % QW] = acc;
  part_count[part][lane % QW] = cnt;
  part_nan[part][lane % QW] = nans;
  part_above[part][lane % QW] = abv;
  __syncthreads();
  if (tid < QW && q_in) {                                    // tid < QW: lane % QW == tid, this thread's own row
    double a = 0.0;
    int32_t c = 0, n = 0, b = 0;
    if (q_on) {
#pragma unroll
      for (int p = 0; p < NW * SL; ++p) {                    // the fixed order of a row's partials
        a += part_sum[p][tid];
        c += part_count[p][tid];
        n += part_nan[p][tid];
        b += part_above[p][tid];
      }
    }
    sum[row] = a;
    count[row] = c;
    nan[row] = n;
    if (above != nullptr) above[row] = b;
  }
}

}  // namespace

extern "C" int mhs_pair_key_tile(void) { return KT; }

extern "C" int mhs_msim_pair_stats(const float* q, int64_t nq, const float* k, int64_t nk, const int32_t* q_valid, const int32_t* k_valid,
                                   const int32_t* q_group, const int32_t* k_group, int self, float threshold, double* sum, int32_t* count,
                                   int32_t* nan, int32_t* above, mh_stream_t stream) {
  constexpr int64_t kMaxRows = 0x7fffffffLL / D;            // n * 56 is a 32-bit element index in the kernel
  MH_CHECK_ARG(q && k && sum && count && nan, "msim_pair_stats: q, k, sum, count and nan must not be NULL");
  MH_CHECK_ARG(nq >= 1 && nq <= kMaxRows && nk >= 1 && nk <= kMaxRows, "msim_pair_stats: nq = %lld, nk = %lld outside 1..%lld",
               (long long)nq, (long long)nk, (long long)kMaxRows);
  MH_CHECK_ARG(self == 0 || self == 1, "msim_pair_stats: self = %d is neither 0 nor 1", self);
  MH_CHECK_ARG(!self || (q == k && nq == nk && q_valid == k_valid && q_group == k_group),
               "msim_pair_stats: self = 1 needs q == k, nq == nk and the same validity and group pointers");
  // the fewest slices per wave (the most query rows per block: the least LDS traffic per pair) that still give every CU a block
  const int64_t cus = mh_device_cus();
  const int sl = (nq + 63) / 64 >= cus ? 1 : (nq + 31) / 32 >= cus ? 2 : 4;
  const dim3 grid((unsigned)((nq + 64 / sl - 1) / (64 / sl)));
  mh_prof_note("nq=%lld nk=%lld slices=%d self=%d", (long long)nq, (long long)nk, sl, self);
  if (sl == 1)
    MH_LAUNCH(msim_pair_stats_kernel<1>, grid, dim3(TB), 0, (hipStream_t)stream, q, (int)nq, k, (int)nk, q_valid, k_valid, q_group, k_group,
              self, threshold, sum, count, nan, above);
  else if (sl == 2)
    MH_LAUNCH(msim_pair_stats_kernel<2>, grid, dim3(TB), 0, (hipStream_t)stream, q, (int)nq, k, (int)nk, q_valid, k_valid, q_group, k_group,
              self, threshold, sum, count, nan, above);
  else
    MH_LAUNCH(msim_pair_stats_kernel<4>, grid, dim3(TB), 0, (hipStream_t)stream, q, (int)nq, k, (int)nk, q_valid, k_valid, q_group, k_group,
              self, threshold, sum, count, nan, above);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
