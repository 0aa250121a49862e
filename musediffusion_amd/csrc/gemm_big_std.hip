// The 256x128 big tile (two blocks per CU) with the generic epilogue (EPI 0): bias / activation / residual in its fixed forms, dropout, and the
// deferred-LayerNorm kernels.
#include "gemm_big.h"

namespace mhgemm __attribute__((visibility("hidden"))) {

template int launch_big<CfgStd, 0>(const GemmArgs&, hipStream_t, int);

}  // namespace mhgemm
