// gemm_glds_kernel<.., CONV = false, ..>: the GEMM instantiations of the LDS-DMA kernel (gemm_glds_kernel.h)
#include "gemm_glds_kernel.h"

namespace crg_mm {
KernFn pick_glds_gemm(const crg_plan::Launch& L) { return pick_glds_unit<false>(L); }
}  // namespace crg_mm
