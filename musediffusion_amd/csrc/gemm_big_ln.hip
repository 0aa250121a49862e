// Bias + residual + LayerNorm over complete rows (EPI 3): the big tile whose width is the whole output row - 256x128 (N = 128), 256x256
// ping-pong (N = 256), 128x512 ping-pong (N = 512).  The plain-loop and 64-row forms the last one was measured against exist in the debug
// library only (mh_gemm_set_plain_stores bits 2 - 4).
#include "gemm_big.h"

namespace mhgemm __attribute__((visibility("hidden"))) {

template int launch_big<CfgStd, 3>(const GemmArgs&, hipStream_t, int);
template int launch_big<CfgWidePP, 3>(const GemmArgs&, hipStream_t, int);
template int launch_big<CfgRowPP, 3>(const GemmArgs&, hipStream_t, int);
#ifdef MH_ABLATE
template int launch_big<CfgRow, 3>(const GemmArgs&, hipStream_t, int);
template int launch_big<CfgRow64, 3>(const GemmArgs&, hipStream_t, int);
#endif

}  // namespace mhgemm
