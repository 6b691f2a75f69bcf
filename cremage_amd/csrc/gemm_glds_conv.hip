// gemm_glds_kernel<.., CONV = true, ..>: the implicit-GEMM conv instantiations of the LDS-DMA kernel (gemm_glds_kernel.h)
#include "gemm_glds_kernel.h"

namespace crg_mm {
KernFn pick_glds_conv(const crg_plan::Launch& L) { return pick_glds_unit<true>(L); }
}  // namespace crg_mm
