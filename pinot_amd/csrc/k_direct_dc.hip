// k_direct_dc.hip — the direct-load scan kernel's instances for plans with DISTINCTCOUNT aggregations (SLOT_DISTINCT
// slots and their side bitmaps, KParamsDc), one accumulator mode per object (compiled with -DPGPU_MODE=0|1: such
// plans have dense key spaces).
#include "scan_direct.h"

#ifndef PGPU_MODE
#error "compile with -DPGPU_MODE=0 (LDS) or 1 (GLOBAL)"
#endif
#if PGPU_MODE != 0 && PGPU_MODE != 1
#error "the DC instances exist for MODE_LDS and MODE_GLOBAL only"
#endif
#define PGPU_CAT2(a, b) a##b
#define PGPU_CAT(a, b) PGPU_CAT2(a, b)

namespace pgpu {

// variant: kVariantDcSparse or kVariantDcDense.
int PGPU_CAT(launch_direct_dc_mode, PGPU_MODE)(const KParamsDc& p, int variant, int grid, size_t lds_bytes, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (variant == kVariantDcDense)
    hipLaunchKernelGGL((filter_groupby_dc_kernel<PGPU_MODE, true>), dim3(grid), dim3(kBlock), lds_bytes, s, p);
  else
    hipLaunchKernelGGL((filter_groupby_dc_kernel<PGPU_MODE, false>), dim3(grid), dim3(kBlock), lds_bytes, s, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int PGPU_CAT(occupancy_direct_dc_mode, PGPU_MODE)(int variant, size_t lds_bytes) {
  int n = 0;
  const hipError_t e =
      variant == kVariantDcDense
          ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filter_groupby_dc_kernel<PGPU_MODE, true>, kBlock, lds_bytes)
          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, filter_groupby_dc_kernel<PGPU_MODE, false>, kBlock,
                                                         lds_bytes);
  return e == hipSuccess ? n : -1;
}

}  // namespace pgpu
