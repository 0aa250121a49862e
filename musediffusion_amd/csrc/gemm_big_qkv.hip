// The QKV projection with head scatter (EPI 1) on the 256x128 and 256x256 big tiles.
#include "gemm_big.h"

namespace mhgemm __attribute__((visibility("hidden"))) {

template int launch_big<CfgStd, 1>(const GemmArgs&, hipStream_t, int);
template int launch_big<CfgWide, 1>(const GemmArgs&, hipStream_t, int);

}  // namespace mhgemm
