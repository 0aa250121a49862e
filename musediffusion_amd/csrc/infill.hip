// Infill on the device (include/musehip_infill.h): the mask that selects the interiors of a bar range - or single note fields inside
// it - of ragged token rows, with room for new notes, and the splice that brings a sampled row back: the original tokens outside the
// region bit for bit, whole well-formed notes inside it.  Not in the reference: its only edit (run/sample.py, modification mode)
// re-noises the whole note region.  One 256-thread block per row, the row in LDS (at most mh_batch_max_row() tokens); bar ordinals and
// compaction offsets come from ballot scans over chunks of 256 tokens.  Integer byte movers: no MFMA shape here on purpose.
#include "common.h"
#include "../../include/musehip_infill.h"

namespace {

constexpr int TB = 256;
constexpr int MAX_ROW = 4096;      // == mh_batch_max_row() (batch.hip); the wrappers check it
constexpr int32_t EOS = 1, BAR = 2;

// position 0, velocity 1, pitch 2, duration 3; everything else -1
__device__ __forceinline__ int token_class(int32_t t) {
  if (t >= 432 && t <= 559) return 0;
  if (t >= 131 && t <= 194) return 1;
  if (t >= 3 && t <= 130) return 2;
  if (t >= 304 && t <= 431) return 3;
  return -1;
}

// exclusive prefix sum of one flag per thread over the block (256 threads = 4 waves); the block total to every thread
__device__ __forceinline__ int block_excl_scan(bool flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  const int before = __builtin_popcountll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __builtin_popcountll(m);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + before;
}

__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int block_min(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = red[w] < r ? red[w] : r;
  __syncthreads();
  return r;
}

// the quad a token of class c at index i belongs to starts at i - c: four tokens of classes 0, 1, 2, 3 inside [0, n)
__device__ __forceinline__ bool quad_at(const int32_t* row, int q, int n) {
  if (q < 0 || q + 3 >= n) return false;
  return token_class(row[q]) == 0 && token_class(row[q + 1]) == 1 && token_class(row[q + 2]) == 2 && token_class(row[q + 3]) == 3;
}

__global__ __launch_bounds__(TB) void infill_plan_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ prefix_mask,
                                                        const int32_t* __restrict__ bar_lo, const int32_t* __restrict__ bar_hi, int room,
                                                        int fields, int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_mask,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ info, int L) {
  __shared__ int32_t tok[MAX_ROW];    // the row
  __shared__ int32_t otok[MAX_ROW];   // the widened row
  __shared__ uint8_t omask[MAX_ROW];  // and its mask
  __shared__ int wsum[4];
  __shared__ int red[4];
  __shared__ int p_lo_s, p_hi_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t row = (int64_t)b * L;

  // ---- everything the status depends on, before anything is written
  int first_nz = L, not_one = 0;      // the first index with mask != 0; 1 + the last index with mask != 1
  for (int j = tid; j < L; j += TB) {
    tok[j] = tokens[row + j];
    const int32_t mk = prefix_mask[row + j];
    if (mk != 0 && j < first_nz) first_nz = j;
    if (mk != 1) not_one = j + 1;
  }
  const int m = block_min(first_nz, red);                            // (its barriers also publish tok[])
  const int ones_from = -block_min(-not_one, red);                   // the mask is m zeros, then ones, iff ones_from <= m
  int first_eos = L;
  for (int j = tid; j < L; j += TB)
    if (j >= m && tok[j] == EOS && j < first_eos) first_eos = j;
  const int e = block_min(first_eos, red);
  int c = 0;
  for (int j = m + tid; j < e; j += TB) c += tok[j] == BAR;
  const int nb = block_sum(c, red);
  const int lo = bar_lo[b], hi = bar_hi[b];
  const bool whole = fields == 15;
  int st = MHI_OK;
  long long added64 = 0;
  if (!(ones_from <= m && m > 0 && m < L)) st = MHI_BAD_MASK;
  else if (e >= L) st = MHI_NO_EOS;
  else if (!(lo >= 0 && lo < hi && hi <= nb)) st = MHI_BAD_RANGE;
  else {
    added64 = whole ? 4ll * room * (hi - lo) : 0;
    if (e + 1 + added64 > L) st = MHI_OVERFLOW;
  }
  if (st != MHI_OK) {                                                // uniform
    for (int j = tid; j < L; j += TB) {
      out_tokens[row + j] = tok[j];
      out_mask[row + j] = 0;
    }
    if (tid == 0) status[b] = st;
    if (tid < 4) info[b * 4 + tid] = 0;
    return;
  }
  const int added = (int)added64, g = added / (hi - lo);             // g (hi - lo) <= L

  // ---- the widened row: a slot no original token lands on is an inserted one (pad, selected)
  for (int j = tid; j < L; j += TB) {
    otok[j] = 0;
    omask[j] = 1;
  }
  if (tid == 0) p_hi_s = e;                                          // p_nb := e
  __syncthreads();
  int carry = 0;
  for (int j0 = 0; j0 < L; j0 += TB) {
    const int j = j0 + tid;
    const bool in = j < L, inside = in && j >= m && j < e;
    const bool isbar = inside && tok[j] == BAR;
    int total;
    const int k = carry + block_excl_scan(isbar, wsum, total) + (int)isbar - 1;   // the bar j lies in or opens; -1 before p_0
    carry += total;
    if (!in) continue;
    if (isbar && k == lo) p_lo_s = j;
    if (isbar && k == hi) p_hi_s = j;
    const bool sel = inside && !isbar && k >= lo && k < hi;
    // selected bars that end at or before j: their insertions sit in front of it
    int ended = j >= e ? hi - lo : (k < hi ? k : hi) - lo;
    if (ended < 0) ended = 0;
    const int nj = j + g * ended;                                    // strictly increasing in j
    bool mk = sel;
    if (!whole && sel) {
      // the quad's tokens have classes >= 0: none is a BAR or the EOS, so all four lie in j's interior
      const int cl = token_class(tok[j]);
      mk = cl >= 0 && ((fields >> cl) & 1) && quad_at(tok, j - cl, L);
    }
    if (nj < L) {
      otok[nj] = tok[j];
      omask[nj] = mk;
    }
  }
  __syncthreads();
  int n_mask = 0;
  for (int j = tid; j < L; j += TB) {
    out_tokens[row + j] = otok[j];
    out_mask[row + j] = omask[j];
    n_mask += omask[j];
  }
  n_mask = block_sum(n_mask, red);
  if (tid == 0) {
    status[b] = MHI_OK;
    info[b * 4 + 0] = p_lo_s + 1;
    info[b * 4 + 1] = p_hi_s + added;
    info[b * 4 + 2] = n_mask;
    info[b * 4 + 3] = added;
  }
}

__global__ __launch_bounds__(TB) void infill_splice_kernel(const int32_t* __restrict__ sampled, const int32_t* __restrict__ plan_tokens,
                                                          const int32_t* __restrict__ plan_mask, const int32_t* __restrict__ status,
                                                          int fields, int32_t* __restrict__ out, int32_t* __restrict__ counts, int L) {
  __shared__ int32_t kept_tok[MAX_ROW];   // the row after stage (a)
  __shared__ uint8_t region[MAX_ROW];     // 1: the token came from a plan_mask == 1 slot
  __shared__ int wsum[4];
  __shared__ int red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t row = (int64_t)b * L;
  if (status[b] != MHI_OK) {                                         // uniform
    for (int j = tid; j < L; j += TB) out[row + j] = plan_tokens[row + j];
    if (tid < 4) counts[b * 4 + tid] = 0;
    return;
  }
  int kept = 0, pads = 0, other = 0, changed = 0;
  if (fields != 15) {
    for (int j = tid; j < L; j += TB) {
      int32_t v = plan_tokens[row + j];
      if (plan_mask[row + j] != 0) {
        const int32_t s = sampled[row + j];
        if (token_class(s) == token_class(v)) {
          ++kept;
          changed += s != v;
          v = s;
        } else {
          ++other;
        }
      }
      out[row + j] = v;
    }
  } else {
    // (a) drop the region slots that hold a pad or no note token
    int n1 = 0;
    for (int j0 = 0; j0 < L; j0 += TB) {
      const int j = j0 + tid;
      bool keep = false, reg = false;
      int32_t v = 0;
      if (j < L) {
        reg = plan_mask[row + j] != 0;
        v = reg ? sampled[row + j] : plan_tokens[row + j];
        const bool pad = reg && v == 0, stray = reg && v != 0 && token_class(v) < 0;
        pads += pad;
        other += stray;
        keep = !pad && !stray;
      }
      int total;
      const int at = n1 + block_excl_scan(keep, wsum, total);
      if (keep) {                                                    // at < L
        kept_tok[at] = v;
        region[at] = reg;
      }
      n1 += total;
    }
    __syncthreads();
    // (b) of the region tokens only whole quads survive
    int n2 = 0;
    for (int i0 = 0; i0 < n1; i0 += TB) {
      const int i = i0 + tid;
      bool keep = false, reg = false;
      int32_t v = 0;
      if (i < n1) {
        v = kept_tok[i];
        reg = region[i];
        keep = true;
        if (reg) {
          const int q = i - token_class(v);                          // a region token here has a class >= 0
          keep = quad_at(kept_tok, q, n1) && region[q] && region[q + 1] && region[q + 2] && region[q + 3];
          other += !keep;
          kept += keep;
        }
      }
      int total;
      const int at = n2 + block_excl_scan(keep, wsum, total);
      if (keep) out[row + at] = v;                                   // at <= i < L
      n2 += total;
    }
    for (int j = n2 + tid; j < L; j += TB) out[row + j] = 0;
  }
  kept = block_sum(kept, red);
  pads = block_sum(pads, red);
  other = block_sum(other, red);
  changed = block_sum(changed, red);
  if (tid == 0) {
    counts[b * 4 + 0] = kept;
    counts[b * 4 + 1] = pads;
    counts[b * 4 + 2] = other;
    counts[b * 4 + 3] = changed;
  }
}

}  // namespace

extern "C" int mhi_infill_plan(const int32_t* tokens, const int32_t* prefix_mask, const int32_t* bar_lo, const int32_t* bar_hi, int room,
                               int fields, int32_t* out_tokens, int32_t* out_mask, int32_t* status, int32_t* info, int B, int L,
                               mh_stream_t stream) {
  MH_CHECK_ARG(tokens && prefix_mask && bar_lo && bar_hi && out_tokens && out_mask && status && info && B > 0,
               "infill_plan: bad arguments (a NULL pointer or B < 1)");
  MH_CHECK_ARG(L >= 1 && L <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "infill_plan: rows of 1..%d tokens (got L = %d)", MAX_ROW, L);
  MH_CHECK_ARG(room >= 0 && fields >= 1 && fields <= 15, "infill_plan: room >= 0 and fields in 1..15 (got room = %d, fields = %d)", room,
               fields);
  MH_CHECK_ARG(fields == 15 || room == 0, "infill_plan: room is for whole notes (fields = 15), got room = %d with fields = %d", room,
               fields);
  MH_LAUNCH(infill_plan_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, tokens, prefix_mask, bar_lo, bar_hi, room, fields, out_tokens,
            out_mask, status, info, L);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mhi_infill_splice(const int32_t* sampled, const int32_t* plan_tokens, const int32_t* plan_mask, const int32_t* status,
                                 int fields, int32_t* out, int32_t* counts, int B, int L, mh_stream_t stream) {
  MH_CHECK_ARG(sampled && plan_tokens && plan_mask && status && out && counts && B > 0,
               "infill_splice: bad arguments (a NULL pointer or B < 1)");
  MH_CHECK_ARG(L >= 1 && L <= MAX_ROW && MAX_ROW == mh_batch_max_row(), "infill_splice: rows of 1..%d tokens (got L = %d)", MAX_ROW, L);
  MH_CHECK_ARG(fields >= 1 && fields <= 15, "infill_splice: fields in 1..15 (got %d)", fields);
  MH_LAUNCH(infill_splice_kernel, dim3(B), dim3(TB), 0, (hipStream_t)stream, sampled, plan_tokens, plan_mask, status, fields, out, counts,
            L);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
