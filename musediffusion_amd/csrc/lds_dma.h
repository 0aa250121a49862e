// lds_dma.h - the stage-DMA idioms every hot kernel family is built on, spelled once: a ring of LDS stages filled by LDS-DMA in 1-KiB
// pieces (16 rows x 64 B), counted `s_waitcnt vmcnt` waits, LDS rows of 64 B with the chunk swizzle MH_GSW, and - for K32-panel operands -
// a buffer descriptor per operand.  Device-only and __forceinline__; a kernel's main loop stays written out in its own file and takes
// only these pieces from here (the XCD-aware block order, mh_xcd_remap, is in common.h).
#pragma once
#include "common.h"

// ---- waits.  vmcnt counts this wave's vector-memory operations (DMA pieces and stores alike) in issue order.
template <int N> __device__ __forceinline__ void mh_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// wait until all but the youngest `stages` DMA stages (PIECES loads each) of this wave have landed; EXTRA = vector-memory
// operations of another kind (the previous tile's epilogue stores) issued after the awaited stage; DEPTH = the largest `stages`
// told apart (a ring of DEPTH + 1 stages never has more in flight behind the awaited one)
template <int PIECES, int EXTRA = 0, int DEPTH = 3> __device__ __forceinline__ void mh_wait_stages(int stages) {
  static_assert(DEPTH >= 1 && DEPTH <= 3, "one rung per stage in flight, up to three");
  static_assert(DEPTH * PIECES + EXTRA <= 63, "vmcnt is a 6-bit counter");
  if (stages >= DEPTH) mh_wait_vmcnt<DEPTH * PIECES + EXTRA>();
  else if (DEPTH > 2 && stages == 2) mh_wait_vmcnt<2 * PIECES + EXTRA>();
  else if (DEPTH > 1 && stages == 1) mh_wait_vmcnt<PIECES + EXTRA>();
  else mh_wait_vmcnt<EXTRA>();
}
// lgkmcnt(0): this wave's LDS reads and writes are done.  Two forms that are NOT interchangeable: the builtin is only the
// instruction, and the compiler still moves memory operations across it; the asm form is a compiler barrier as well (before an
// s_barrier that publishes LDS writes to other waves).
__device__ __forceinline__ void mh_wait_lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }   // vmcnt 63, expcnt 7, lgkmcnt 0
__device__ __forceinline__ void mh_wait_lgkmcnt0_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- LDS-DMA issue: 16 bytes per lane, i.e. one 1-KiB piece per wave.  A wave's lanes land at consecutive 16-byte slots from the
// LDS address of lane 0 on.  AUX = the instruction's cache-policy bits (2: nt); IMM = its immediate byte offset, which advances the
// LDS address as well as the buffer address (both are literals in the encoding, hence template arguments).
template <int AUX = 0> __device__ __forceinline__ void mh_glds16(const void* global_src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)global_src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, AUX);
}
template <int IMM, int AUX = 0> __device__ __forceinline__ void mh_buf_lds16(__amdgpu_buffer_rsrc_t rsrc, void* lds_dst, int voffset, int soffset) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, voffset, soffset, IMM, AUX);
}

// ---- LDS rows of 64 B = 4 chunks of 16 B: logical chunk c of row r is stored at physical chunk c ^ MH_GSW[(r >> 2) & 3], so that every
// 16-lane group of a ds_read_b128 fragment read hits 16 distinct 16-B slots.  The DMA writes LDS linearly, so the issuing lane applies the
// swizzle to its global SOURCE address.
constexpr int MH_GSW[4] = {0, 2, 3, 1};

// ---- buffer descriptors.  Word 3 of a raw buffer descriptor: DATA_FORMAT = 32 bits, stride 0, no index - offsets are bytes, checked
// against the descriptor's byte count; a load beyond it returns zeros.
constexpr int MH_RSRC_FLAGS = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mh_buf_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(base)), 0, bytes, MH_RSRC_FLAGS);
}
// The descriptor of a row window of a K32-panel operand ([npanels][ld rows][32] 2-byte elements: row r of panel p at byte (p ld + r) 64):
// it starts at row `row0` of panel 0 and ends with the rows the operand OWNS in its last panel (`rows`; `base` may itself be a row
// window of a larger panel buffer: ld > rows, first row > 0).  Rows beyond `rows` are not clamped by the kernels: inside the buffer
// they read other rows (their outputs are never stored), in the last panel they are zero-filled by the bound instead of being fetched
// from behind the allocation.  The host checks mh_panel_desc_fits (common.h): the byte count is 31 bits.
// (The arguments stand in the order in which the expression reads them, which is the order the call sites' operands are evaluated in:
// with `rows` ahead of `npanels` hipcc schedules the scalar prologue of split_gemm_kernel differently.  The bf16 GEMM kernels, whose
// K / 32 - 1 is a 32-bit subtraction, spell the same bound out over mh_buf_rsrc: behind a function boundary the compiler folds the
// sum another way and their register counts change - profiles/dma_primitives_isa_and_bench.txt.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mh_panel_rsrc(const void* base, int64_t row0, int64_t npanels, int64_t ld, int64_t rows) {
  return mh_buf_rsrc(reinterpret_cast<const char*>(base) + row0 * 64, (int)((npanels - 1) * ld * 64 + (rows - row0) * 64));
}
