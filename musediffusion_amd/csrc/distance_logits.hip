// Token cross-entropy over the logits of logits_mode 2 (models/network.py:94-104; _token_discrete_loss, models/diffusion.py:556-575):
// the score of position n against lm_head row v is the negative Euclidean distance
//     d2 = (wn[v] + xn[n]) - 2 dot[n][v],   s = -sqrtf(fmaxf(d2, 0))
// - distance_scores_kernel's expression (elementwise.hip), the reference's association of the three terms; this file compiles without FP
// contraction like that one.  dot = x W^T arrives as the fp32 GEMM's output [N][ld] (ld >= V, columns V .. ld - 1 are padding: never
// read into a maximum or a sum), wn / xn from mh_row_sqnorm.  The [N, V] score tensor never exists in memory: forward and backward
// recompute s from the product, one wave per row like ce_fwd_kernel / ce_bwd_kernel (train.hip).
//
// Backward.  With p = exp(s - lse) and dl = g (p - [v == id]) the gradient with respect to d2 is G = dl / (2 s) for s < 0, from which
//     d_dots = -2 G,   d_xn[n] = sum_v G[n][v],   d_wn[v] = sum_n G[n][v] = -1/2 colsum(d_dots)   (mh_col_sum)
// and d|x|^2 / dx = 2 x (mh_sqnorm_bwd) carries d_xn / d_wn on to x and W.
// WHERE THE CLAMP IS ACTIVE (d2 <= 0, s == 0) G IS 0.  This differs from the reference on purpose: torch's autograd gives 0 below the clamp
// but inf / NaN at d2 == 0 exactly (the derivative of sqrt at 0) - a position that sits on an embedding row, which the decoder-NLL term
// of training_losses approaches (x_start = W[id] + 0.01 noise), would poison the whole training step.
#include <math.h>
#include <stdlib.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float distance_score(float wn, float xn, float dot) {
  const float d2 = (wn + xn) - 2.0f * dot;
  return -sqrtf(fmaxf(d2, 0.0f));
}

__global__ void distance_ce_fwd_kernel(const float* __restrict__ dots, int64_t ld, const float* __restrict__ wn, const float* __restrict__ xn,
                                       const int32_t* __restrict__ ids, float* __restrict__ nll, float* __restrict__ lse, int64_t n, int V) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* p = dots + row * ld;
  const float xr = xn[row];
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, distance_score(wn[c], xr, p[c]));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < V; c += 64) sum += expf(distance_score(wn[c], xr, p[c]) - mx);
  sum = wave_sum(sum);
  const float l = mx + logf(sum);
  if (lane == 0) {
    const int t = ids[row];
    lse[row] = l;
    // (the host entry point refuses an id outside [0, V) before the launch; inside a stream capture it cannot look, and then no read
    // happens here either)
    nll[row] = (t >= 0 && t < V) ? l - distance_score(wn[t], xr, p[t]) : NAN;
  }
}

__global__ void distance_ce_bwd_kernel(const float* __restrict__ dots, int64_t ld, const float* __restrict__ wn, const float* __restrict__ xn,
                                       const int32_t* __restrict__ ids, const float* __restrict__ lse, const float* __restrict__ g,
                                       float* __restrict__ d_dots, float* __restrict__ d_xn, int64_t n, int V) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* p = dots + row * ld;
  float* d = d_dots + row * ld;
  const float xr = xn[row], l = lse[row], gs = g[row];
  const int t = ids[row];
  float acc = 0.f;   // this lane's columns in ascending order, then the wave tree: the same order on every run
  for (int c = lane; c < (int)ld; c += 64) {
    float G = 0.f;
    if (c < V) {
      const float s = distance_score(wn[c], xr, p[c]);
      if (s < 0.f) {
        const float dl = gs * (expf(s - l) - (c == t ? 1.f : 0.f));
        G = dl / (2.0f * s);
      }
      acc += G;
    }
    d[c] = -2.0f * G;
  }
  acc = wave_sum(acc);
  if (lane == 0) d_xn[row] = acc;
}

// out[r][:] = 2 (c_scale c[r]) x[r][:] - the backward of mh_row_sqnorm
__global__ void sqnorm_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ c, float c_scale, float* __restrict__ out,
                                  int64_t ldo, int64_t rows, int cols) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int e = (int)(i - r * cols);
    out[r * ldo + e] = 2.0f * (c_scale * c[r]) * x[r * ldx + e];
  }
}

}  // namespace

extern "C" int mh_distance_ce_fwd(const float* dots, int64_t ld, const float* w_sqnorm, const float* x_sqnorm, const int32_t* ids, float* nll,
                                  float* lse, int64_t n, int V, mh_stream_t stream) {
  MH_CHECK_ARG(dots && w_sqnorm && x_sqnorm && ids && nll && lse && n > 0 && V > 0 && ld >= V, "distance_ce_fwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  // an id outside [0, V) is the caller's error, found here and not by a device read: the ids come to the host (4 n bytes, stream-ordered).
  // A capturing stream cannot be waited on; there the kernel's own guard stands alone
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  if (cap == hipStreamCaptureStatusNone) {
    int32_t* host = static_cast<int32_t*>(malloc((size_t)n * sizeof(int32_t)));
    MH_CHECK_ARG(host, "distance_ce_fwd: out of host memory");
    hipError_t e = hipMemcpyAsync(host, ids, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int64_t bad = -1;
    if (e == hipSuccess)
      for (int64_t i = 0; i < n; ++i)
        if (host[i] < 0 || host[i] >= V) { bad = i; break; }
    const int32_t bad_id = bad >= 0 ? host[bad] : 0;
    free(host);
    MH_HIP(e);
    MH_CHECK_ARG(bad < 0, "distance_ce_fwd: ids[%lld] = %d is outside [0, %d)", (long long)bad, bad_id, V);
  }
  MH_LAUNCH(distance_ce_fwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, dots, ld, w_sqnorm, x_sqnorm, ids, nll, lse, n, V);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_distance_ce_bwd(const float* dots, int64_t ld, const float* w_sqnorm, const float* x_sqnorm, const int32_t* ids,
                                  const float* lse, const float* grad, float* d_dots, float* d_xn, int64_t n, int V, mh_stream_t stream) {
  MH_CHECK_ARG(dots && w_sqnorm && x_sqnorm && ids && lse && grad && d_dots && d_xn && n > 0 && V > 0 && ld >= V && ld <= INT32_MAX,
               "distance_ce_bwd: bad arguments");
  MH_LAUNCH(distance_ce_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dots, ld, w_sqnorm, x_sqnorm, ids, lse,
            grad, d_dots, d_xn, n, V);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_sqnorm_bwd(const float* x, int64_t ldx, const float* c, float c_scale, float* out, int64_t ldo, int64_t rows, int cols,
                             mh_stream_t stream) {
  MH_CHECK_ARG(x && c && out && rows > 0 && cols > 0 && ldx >= cols && ldo >= cols, "sqnorm_bwd: bad arguments");
  const int64_t blocks = (rows * cols + 255) / 256;
  MH_LAUNCH(sqnorm_bwd_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream, x, ldx, c, c_scale, out, ldo,
            rows, cols);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
