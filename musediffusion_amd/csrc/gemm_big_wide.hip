// The 256x256 big tile (one block per CU) with the generic epilogue (EPI 0): row-major launches that fill the chip with it.
#include "gemm_big.h"

namespace mhgemm __attribute__((visibility("hidden"))) {

template int launch_big<CfgWide, 0>(const GemmArgs&, hipStream_t, int);

}  // namespace mhgemm
