// Dataset loader on the device (include/musehip_data.h): the three kernels that turn a resident, merged ComMU dataset into a training
// batch.  Reference: MuseDiffusion/data/__init__.py:14-89 (load_data_music), data/wrapper.py:42-87 (MidiSequenceDataset.__getitem__:
// one row at a time through the DataLoader), commu/preprocessor/augment.py:35-98 + utils/utils.py:37-96 (key / tempo augmentation,
// done there on MIDI files before encoding; here a token map on merged rows).  Conventions of batch.hip: ragged rows
// (`values`, `offsets[B + 1]` int64), one 256-thread block per row, rows of up to mh_batch_max_row() tokens where a row is staged in
// LDS.  Integer byte movers - HBM / latency bound, no MFMA shape.
#include "common.h"

#include "../../include/musehip_data.h"

namespace {

constexpr int TB = 256;
constexpr int MAX_ROW = 4096;   // == mh_batch_max_row() (batch.hip); checked at the launch site

// length of source row i, 0 for an index outside [0, n) or offsets that run backwards (clamped to int32)
__device__ __forceinline__ long long src_row_len(const int64_t* __restrict__ src_offsets, int64_t n, int64_t i) {
  if (i < 0 || i >= n) return 0;
  const long long d = (long long)(src_offsets[i + 1] - src_offsets[i]);
  return d < 0 ? 0 : (d > 0x7fffffffLL ? 0x7fffffffLL : d);
}

// lengths, their exclusive scan and the statuses in one block: out_offsets[b + 1] = sum of length[..b] while the sum fits cap; the
// rows behind that get length 0 and OVERFLOW (the scheme of encode.hip's merge_offsets_kernel)
__global__ __launch_bounds__(TB) void gather_offsets_kernel(const int64_t* __restrict__ src_offsets, int64_t n, const int64_t* __restrict__ idx,
                                                           int64_t* __restrict__ out_offsets, int32_t* __restrict__ length,
                                                           int32_t* __restrict__ status, int B, int64_t cap) {
  __shared__ long long wtot[4];
  __shared__ long long fit_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long run = 0;
  if (tid == 0) { out_offsets[0] = 0; fit_s = 0; }
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += TB) {
    const int b = b0 + tid;
    long long len = 0;
    bool bad = false;
    if (b < B) {
      const int64_t i = idx[b];
      bad = i < 0 || i >= n;
      len = src_row_len(src_offsets, n, i);
    }
    long long incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += wtot[w];
    incl += run;
    run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    // the sums are monotone: once one passes cap every later one does, so the largest that fits is the last before the cut
    const bool fits = incl <= (long long)cap;
    if (b < B && fits) atomicMax((unsigned long long*)&fit_s, (unsigned long long)incl);
    __syncthreads();   // fit_s complete for this chunk (and wtot free for the next)
    if (b < B) {
      out_offsets[b + 1] = fits ? incl : fit_s;
      length[b] = fits ? (int32_t)len : 0;
      status[b] = bad ? MHD_GATHER_BAD_INDEX : (!fits && len > 0) ? MHD_GATHER_OVERFLOW : MHD_GATHER_OK;
    }
  }
}

__global__ __launch_bounds__(TB) void gather_rows_kernel(const int32_t* __restrict__ src_values, const int64_t* __restrict__ src_offsets, int64_t n,
                                                        const int64_t* __restrict__ idx, const int64_t* __restrict__ out_offsets,
                                                        const int32_t* __restrict__ length, int32_t* __restrict__ out, int64_t cap) {
  const int b = blockIdx.x;
  const int64_t i = idx[b], o = out_offsets[b];
  long long len = length[b];
  const long long have = src_row_len(src_offsets, n, i);   // 0 for an index out of range: nothing is read
  if (len > have) len = have;
  if (len <= 0 || o < 0 || o + len > cap) return;          // uniform per block
  const int32_t* __restrict__ s = src_values + src_offsets[i];
  for (int j = threadIdx.x; j < len; j += TB) out[o + j] = s[j];
}

// out may alias a: a row that keeps a is then not touched at all
__global__ __launch_bounds__(TB) void select_rows_kernel(const int32_t* a, const int32_t* __restrict__ bv, const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ take_b, int32_t* out) {
  const int b = blockIdx.x;
  const int64_t off = offsets[b];
  const int64_t len = offsets[b + 1] - off;
  const bool tb = take_b[b] != 0;
  if (!tb && a == out) return;
  const int32_t* s = tb ? bv : a;
  for (int64_t j = threadIdx.x; j < len; j += TB) out[off + j] = s[off + j];
}

__device__ __forceinline__ int mod12(int x) { return ((x % 12) + 12) % 12; }

// the row is staged in LDS, the status is decided by the whole block, and only then is anything written (out may alias values)
__global__ __launch_bounds__(TB) void augment_rows_kernel(const int32_t* values, const int64_t* __restrict__ offsets,
                                                         const int32_t* __restrict__ key_change, const int32_t* __restrict__ bpm_change,
                                                         int32_t* out, int32_t* __restrict__ status) {
  __shared__ int32_t row[MAX_ROW];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t off = offsets[b];
  const int64_t n64 = offsets[b + 1] - off;
  const int k = key_change[b], c = bpm_change[b];
  if (n64 < 12 || n64 > MAX_ROW || k < -6 || k > 5 || c < -2 || c > 2) {   // uniform per block
    if (out != values)
      for (int64_t j = tid; j < n64; j += TB) out[off + j] = values[off + j];
    if (status && tid == 0) status[b] = MHD_AUGMENT_BAD_ROW;
    return;
  }
  const int n = (int)n64;
  int bad_pitch = 0;
  for (int j = tid; j < n; j += TB) {
    const int32_t v = values[off + j];
    row[j] = v;
    if (j >= 11 && v >= 3 && v <= 130 && (v + k < 3 || v + k > 130)) bad_pitch = 1;
  }
  bad_pitch = __syncthreads_or(bad_pitch);   // also: row[] is complete
  const int32_t key = row[1];
  const int st = (key != 602 && key != 623) ? MHD_AUGMENT_NOT_ORIGIN : bad_pitch ? MHD_AUGMENT_PITCH_RANGE : MHD_AUGMENT_OK;
  if (status && tid == 0) status[b] = st;
  for (int j = tid; j < n; j += TB) {
    int32_t v = row[j];
    if (st == MHD_AUGMENT_OK) {
      if (j == 0) {
        if (v >= 561 && v <= 600) {
          const int m = v - 560 + c;
          v = 560 + (m < 1 ? 1 : (m > 40 ? 40 : m));
        }
      } else if (j == 1) {
        if (v >= 602 && v < 614) v = 602 + mod12(v - 602 + k);
        else if (v >= 614 && v < 626) v = 614 + mod12(v - 614 + k);
      } else if (j >= 11) {
        if (v >= 3 && v <= 130) v += k;
        else if (v >= 195 && v < 303) {
          const int r = (v - 195) / 9, q = (v - 195) % 9;
          v = 195 + 9 * mod12(r + k) + q;
        }
      }
    }
    out[off + j] = v;
  }
}

}  // namespace

extern "C" int mhd_gather_offsets(const int64_t* src_offsets, int64_t n, const int64_t* idx, int64_t* out_offsets, int32_t* length,
                                  int32_t* status, int B, int64_t cap, mh_stream_t stream) {
  MH_CHECK_ARG(src_offsets && idx && out_offsets && length && status && n >= 0 && B > 0 && B <= 65536 && cap >= 0,
               "gather_offsets: bad arguments (B in 1..65536)");
  MH_LAUNCH(gather_offsets_kernel, dim3(1), dim3(TB), 0, (hipStream_t)stream, src_offsets, n, idx, out_offsets, length, status, B, cap);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mhd_gather_rows(const int32_t* src_values, const int64_t* src_offsets, int64_t n, const int64_t* idx, const int64_t* out_offsets,
                               const int32_t* length, int32_t* out, int B, int64_t cap, mh_stream_t stream) {
  MH_CHECK_ARG(src_values && src_offsets && idx && out_offsets && length && out && n >= 0 && B > 0 && B <= 65536 && cap >= 0,
               "gather_rows: bad arguments (B in 1..65536)");
  MH_LAUNCH(gather_rows_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, src_values, src_offsets, n, idx, out_offsets, length, out, cap);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mhd_select_rows(const int32_t* a_values, const int32_t* b_values, const int64_t* offsets, const int32_t* take_b, int32_t* out,
                               int B, mh_stream_t stream) {
  MH_CHECK_ARG(a_values && b_values && offsets && take_b && out && B > 0, "select_rows: bad arguments");
  MH_LAUNCH(select_rows_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, a_values, b_values, offsets, take_b, out);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mhd_augment_rows(const int32_t* values, const int64_t* offsets, const int32_t* key_change, const int32_t* bpm_change,
                                int32_t* out, int32_t* status, int B, mh_stream_t stream) {
  MH_CHECK_ARG(values && offsets && key_change && bpm_change && out && B > 0, "augment_rows: bad arguments");
  MH_CHECK_ARG(MAX_ROW == mh_batch_max_row(), "augment_rows: row limit differs from mh_batch_max_row()");
  MH_LAUNCH(augment_rows_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, values, offsets, key_change, bpm_change, out, status);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
