// k_direct_fx.hip — the direct-load scan kernel's instances for plans with fixed-point FLOAT / DOUBLE sums
// (PGPU_OPT_EXACT_FP_SUM, SLOT_SUM_FX slots), one accumulator mode per object (compiled with -DPGPU_MODE=0|1|2).
#include "scan_direct.h"

#ifndef PGPU_MODE
#error "compile with -DPGPU_MODE=0 (LDS), 1 (GLOBAL) or 2 (HASH)"
#endif
#define PGPU_CAT2(a, b) a##b
#define PGPU_CAT(a, b) PGPU_CAT2(a, b)

namespace pgpu {

// variant: kVariantFxSparse or kVariantFxDense.
int PGPU_CAT(launch_direct_fx_mode, PGPU_MODE)(const KParamsFx& p, int variant, int grid, size_t lds_bytes, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (variant == kVariantFxDense)
    hipLaunchKernelGGL((filter_groupby_fx_kernel<PGPU_MODE, true>), dim3(grid), dim3(kBlock), lds_bytes, s, p);
  else
    hipLaunchKernelGGL((filter_groupby_fx_kernel<PGPU_MODE, false>), dim3(grid), dim3(kBlock), lds_bytes, s, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int PGPU_CAT(occupancy_direct_fx_mode, PGPU_MODE)(int variant, size_t lds_bytes) {
  int n = 0;
  const hipError_t e =
      variant == kVariantFxDense
          ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filter_groupby_fx_kernel<PGPU_MODE, true>, kBlock, lds_bytes)
          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filter_groupby_fx_kernel<PGPU_MODE, false>, kBlock,
                                                         lds_bytes);
  return e == hipSuccess ? n : -1;
}

}  // namespace pgpu
