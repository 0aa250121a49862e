// The kernels built on the 256x128 tile's geometry with mfma_32x32x16 and an unrolled K loop: the column-strip FFN1 kernel (gemm_strip.h) and,
// in the debug library, the carried-epilogue experiment it came out of (gemm_carry.h).  They use gemm_big.h's DMA helpers.
#include "gemm_big.h"

namespace mhgemm __attribute__((visibility("hidden"))) {

#include "gemm_strip.h"
#ifdef MH_ABLATE
#ifndef MH_CARRY_VALU
#define MH_CARRY_VALU 6
#endif
#include "gemm_carry.h"
#endif

}  // namespace mhgemm
