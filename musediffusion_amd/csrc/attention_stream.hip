// The streaming attention forward (attn_stream.h: seq_len >= 512, seq_len % 16 == 0, head dim 32 or 64): which instantiation serves a
// problem, the list of the instantiations that are built, and the mh_attention_stream_* entry points.
#include "attn_stream.h"
#ifdef MH_ABLATE
#include "attn_stream_dbg.h"   // attn_stream2_kernel, kStreamDebugOnly
#endif

int mh_drop_args(const mh_dropout* d, DropArgs* out);   // dropout.hip

namespace {

MH_KNOB(int, g_attn_stream, 1);   // A/B mode (mh_attention_set_stream); 1 = the product's rules
MH_KNOB(int, g_attn_abl, 0);      // timing-only ablation of the streaming kernel (mh_attention_set_ablation)

// The instantiations the product picks: stream_choose's results with mode 1 and no ablation, over both head dims
constexpr StreamEntry kStreamProduct[] = {
    MH_STREAM_ENTRY(64, 16, 256, 0, true, true), MH_STREAM_ENTRY(32, 16, 256, 0, true, true),                            // plain, one query block
    MH_STREAM_ENTRY(64, 16, 256, 0, true), MH_STREAM_ENTRY(32, 16, 256, 0, true),                                        // plain, whole stages
    MH_STREAM_ENTRY(64, 16, 256), MH_STREAM_ENTRY(32, 16, 256),                                                          // plain, key-bound
    MH_STREAM_ENTRY(64, 16, 256, 0, true, true, true), MH_STREAM_ENTRY(32, 16, 256, 0, true, true, true),                // pre-scaled, one query block
    MH_STREAM_ENTRY(64, 16, 256, 0, true, false, true), MH_STREAM_ENTRY(32, 16, 256, 0, true, false, true),              // pre-scaled
    MH_STREAM_ENTRY(64, 8, 128, 1), MH_STREAM_ENTRY(32, 8, 256, 1),                                                      // dropout generator
    MH_STREAM_ENTRY(64, 16, 256, 2, true), MH_STREAM_ENTRY(64, 16, 256, 2), MH_STREAM_ENTRY(32, 16, 256, 2),             // dropout bit reader
};

StreamKernel stream_lookup(const StreamVariant& v) {
  for (const StreamEntry& e : kStreamProduct)
    if (e.v == v) return e.kern;
#ifdef MH_ABLATE
  for (const StreamEntry& e : kStreamDebugOnly)
    if (e.v == v) return e.kern;
#endif
  return nullptr;
}

// Which instantiation serves a problem (pure; the arguments were checked by the caller).  mode is mh_attention_set_stream's value, abl
// mh_attention_set_ablation's: the product passes 1 and 0.
//   mode 2: every variant on the 8-wave geometry (not the pre-scaled form, which is built for 16 waves only); 3: the dropout generator on 16
//   waves; 4: the key-bound build on every length; 5 / 6: the grid (stream_grid); 7: attn_stream2_kernel (the caller); 8 / 9 / 10: 128-key
//   stages / static wave priority / both on the one-query-block kernel at head dim 64
StreamVariant stream_choose(int L, int dh, bool dropping, bool bits_in, bool pre, int mode, int abl) {
  StreamVariant v{dh, 16, 256, !dropping ? 0 : bits_in ? 2 : 1, false, false, pre, 0, 0};
  // 16 waves x 256-key stages fill a CU.  8 waves x 64 KiB of stages (128 keys at head dim 64, 256 at 32) is half a CU per block: the in-kernel
  // generator always runs there - its Philox state needs ~30 registers more than the 128 a 16-wave block leaves each wave (the 16-wave build
  // spills 25 dwords per lane); the bit reader needs no generator registers and fits 16 waves
  const bool small = !pre && (mode == 2 || mode == 5 || (v.dropv == 1 && mode != 3));
  if (small) { v.nw = 8; v.sk = dh == 64 ? 128 : 256; }
  const bool whole = L % 256 == 0 && mode != 4;   // no stage or tile is partial
  if (v.dropv == 1) return v;                     // the generator: key-bound body only
  // the bit reader keeps the key-bound body except at head dim 64 on 16 waves (seq_len 1024 of the training configuration): elsewhere its
  // bound-free build spills 60 B per lane and measured 5 % slower, as did staging its keep words in LDS
  if (v.dropv == 2) { v.full = whole && !small && dh == 64; return v; }
  // nt only where ONE block streams a (batch, head)'s keys and values and nobody reads them again (seq_len <= the block's queries): same-box
  // A/B of two builds -1.2 % step time at config 2; with two query blocks per (batch, head) (seq_len 1024) the second reader misses them:
  // +0.4 % on the training step, so the default policy there
  const bool once = !small && L <= v.queries();
  if (pre) { v.full = true; v.kvnt = once; return v; }   // (seq_len % 256 == 0: mh_attention_stream_prescaled_supported)
  v.full = whole;
  v.kvnt = whole && once;
  if (v.kvnt && dh == 64) {
    if (abl) v.abl = abl;
    else if (mode >= 8) { v.sk = mode == 9 ? 256 : 128; v.prio = mode >= 9; }
  }
  return v;
}

// Persistent blocks: as many as fit the chip, or one per item.  Modes 5 / 6 (A/B): the 8-wave geometry on ONE block per CU (each block then
// walks two half-items back to back, the second one's first stage and queries arriving under the first one's tiles, and half of the CU's LDS
// and registers stay free for a block of the other graph branch's kernel) / as many blocks as half the CUs (two items per block)
int stream_grid(const StreamVariant& v, int nitems, int cus, int mode) {
  const int slots = mode == 5 ? cus : mode == 6 ? cus / 2 : cus * v.blocks_per_cu();
  return nitems < slots ? nitems : slots;
}

// The streaming forward with attention-probability dropout: drop->p > 0 needs `keep_bits` (mh_dropout_bits_words(B nh, L) words):
// written by the kernel (bits_in = 0: Philox, the same bits mh_dropout_bits produces) or read from it (bits_in = 1).
int stream_fwd_impl(const void* q, const void* k, const void* vt_perm, void* ctx, int64_t ld_ctx, int ctx_panel, int B, int L, int nh, int dh,
                    float scale, float* lse2, int64_t qsB, int64_t qsH, int64_t qld, const mh_dropout* drop, uint32_t* keep_bits, int bits_in,
                    bool pre, mh_stream_t stream) {
  DropArgs da;
  int rcd = mh_drop_args(drop, &da);
  if (rcd) return rcd;
  const bool dropping = da.thr != 0;
  MH_CHECK_ARG(!dropping || keep_bits, "attention_stream: dropout needs the keep_bits tensor");
  MH_CHECK_ARG(!(pre && dropping), "attention_stream: the pre-scaled form has no dropout variant");
  MH_CHECK_ARG(qld % 8 == 0 && qsH % 8 == 0 && qsB % 8 == 0 && qld >= dh, "attention_stream: q/k strides must be multiples of 8 elements");
  MH_CHECK_ARG(q && k && vt_perm && ctx, "attention_stream: null pointer");
  MH_CHECK_ARG(B > 0 && nh > 0 && mh_attention_stream_supported(L, dh),
               "attention_stream: needs seq_len %% 16 == 0, seq_len >= 512 and head dim 32 or 64 (got L=%d dh=%d)", L, dh);
  MH_CHECK_ARG(ctx_panel || ld_ctx % 4 == 0, "attention_stream: ld_ctx must be a multiple of 4");
  MH_CHECK_ARG(!pre || mh_attention_stream_prescaled_supported(L, dh), "attention_stream(pre-scaled): seq_len %d must be a multiple of 256", L);
  hipStream_t s = (hipStream_t)stream;
  const int cus = mh_device_cus();
  const int nbh = B * nh;
  const float sl2 = scale * 1.4426950408889634f;
  const bf16 *Q = (const bf16*)q, *K = (const bf16*)k, *V = (const bf16*)vt_perm;
#ifdef MH_ABLATE
  // A/B: 64 queries per wave (8 waves, two per SIMD): half the LDS fragment reads per (batch, head)
  if (g_attn_stream == 7 && !pre && !dropping && !lse2 && dh == 64 && L % 512 == 0 &&
      (ctx_panel || (ld_ctx % 8 == 0 && (reinterpret_cast<uintptr_t>(ctx) & 15) == 0))) {
    const auto go2 = L <= 512 ? &launch_stream2<true> : &launch_stream2<false>;   // (nt: as stream_choose's `once`)
    return go2(Q, K, V, (bf16*)ctx, ld_ctx, ctx_panel, L, nh, nbh, sl2, qsB, qsH, qld, cus, s);
  }
#endif
  const StreamVariant v = stream_choose(L, dh, dropping, bits_in != 0, pre, g_attn_stream, g_attn_abl);
  const StreamKernel kern = stream_lookup(v);
  if (!kern) {
    if (v.abl) mh_set_error("attention_stream: ablation %d not built (1 2 4 6 7 8 16 24 31 32 63 95 127 128)", v.abl);
    else mh_set_error("attention_stream: variant dh=%d nw=%d sk=%d dropv=%d full=%d kvnt=%d pre=%d prio=%d not built", v.dh, v.nw, v.sk, v.dropv,
                      (int)v.full, (int)v.kvnt, (int)v.pre, v.prio);
    return MH_ERR_UNSUPPORTED;
  }
  const int bytes = v.lds_bytes(), nitems = nbh * ceil_div(L, v.queries());
  const dim3 grid((unsigned)stream_grid(v, nitems, cus, g_attn_stream)), block(v.block());
  if (int rc = mh_allow_dynamic_lds((const void*)kern, bytes)) return rc;
  mh_prof_note("attn_stream B*nh=%d L=%d dh=%d drop=%d nw=%d sk=%d dropv=%d full=%d kvnt=%d pre=%d items=%d", nbh, L, dh, (int)dropping, v.nw, v.sk,
               v.dropv, (int)v.full, (int)v.kvnt, (int)v.pre, nitems);
  MH_LAUNCH(kern, grid, block, bytes, s, Q, K, V, (bf16*)ctx, ld_ctx, L, nh, nbh, sl2, ctx_panel, lse2, qsB, qsH, qld, da, keep_bits, bits_in);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

}  // namespace

#ifdef MH_ABLATE
extern "C" int mh_attention_set_stream(int on) {
  g_attn_stream = on < 0 ? 0 : (on > 10 ? 10 : on);
  return MH_OK;
}
extern "C" int mh_attention_set_ablation(int bits) {
  g_attn_abl = bits;
  return MH_OK;
}
#endif
extern "C" int mh_attention_stream_enabled(void) { return g_attn_stream; }

extern "C" int mh_attention_stream_supported(int L, int dh) { return L >= 512 && L % 16 == 0 && (dh == 32 || dh == 64); }
// the pre-scaled form is built for whole 256-key stages only (the key-bound variant of it spills)
extern "C" int mh_attention_stream_prescaled_supported(int L, int dh) { return mh_attention_stream_supported(L, dh) && L % 256 == 0; }

extern "C" int mh_attention_stream_fwd_drop(const void* q, const void* k, const void* vt_perm, void* ctx, int64_t ld_ctx, int ctx_panel,
                                            int B, int L, int nh, int dh, float scale, float* lse2, int64_t qsB, int64_t qsH,
                                            int64_t qld, const mh_dropout* drop, uint32_t* keep_bits, int bits_in, mh_stream_t stream) {
  return stream_fwd_impl(q, k, vt_perm, ctx, ld_ctx, ctx_panel, B, L, nh, dh, scale, lse2, qsB, qsH, qld, drop, keep_bits, bits_in, false, stream);
}
// The same forward for queries that carry scale x log2(e) already (mh_gemm_qkv_vtperm_qs): q [B, nh, L, dh]; no dropout
extern "C" int mh_attention_stream_fwd_prescaled(const void* q, const void* k, const void* vt_perm, void* ctx, int64_t ld_ctx, int ctx_panel,
                                                 int B, int L, int nh, int dh, mh_stream_t stream) {
  return stream_fwd_impl(q, k, vt_perm, ctx, ld_ctx, ctx_panel, B, L, nh, dh, 1.0f, nullptr, (int64_t)nh * L * dh, (int64_t)L * dh, dh, nullptr,
                         nullptr, 0, true, stream);
}
extern "C" int mh_attention_stream_fwd_ex(const void* q, const void* k, const void* vt_perm, void* ctx, int64_t ld_ctx, int ctx_panel,
                                          int B, int L, int nh, int dh, float scale, float* lse2, int64_t qsB, int64_t qsH,
                                          int64_t qld, mh_stream_t stream) {
  return mh_attention_stream_fwd_drop(q, k, vt_perm, ctx, ld_ctx, ctx_panel, B, L, nh, dh, scale, lse2, qsB, qsH, qld, nullptr, nullptr, 0, stream);
}
extern "C" int mh_attention_stream_fwd_lse(const void* q, const void* k, const void* vt_perm, void* ctx, int64_t ld_ctx, int ctx_panel,
                                           int B, int L, int nh, int dh, float scale, float* lse2, mh_stream_t stream) {
  return mh_attention_stream_fwd_ex(q, k, vt_perm, ctx, ld_ctx, ctx_panel, B, L, nh, dh, scale, lse2, (int64_t)nh * L * dh, (int64_t)L * dh, dh,
                                    stream);
}
extern "C" int mh_attention_stream_fwd(const void* q, const void* k, const void* vt_perm, void* ctx, int64_t ld_ctx, int ctx_panel,
                                       int B, int L, int nh, int dh, float scale, mh_stream_t stream) {
  return mh_attention_stream_fwd_lse(q, k, vt_perm, ctx, ld_ctx, ctx_panel, B, L, nh, dh, scale, nullptr, stream);
}
