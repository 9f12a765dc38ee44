// k_startree_fx.hip — the star-tree document scan's instance for plans with fixed-point FLOAT / DOUBLE sums
// (PGPU_OPT_EXACT_FP_SUM, SLOT_SUM_FX slots), one accumulator mode per object (compiled with -DPGPU_MODE=0|1|2).
#define PGPU_STAR_SCAN_ONLY 1
#include "startree_kernels.h"

#ifndef PGPU_MODE
#error "compile with -DPGPU_MODE=0 (LDS), 1 (GLOBAL) or 2 (HASH)"
#endif
#define PGPU_CAT2(a, b) a##b
#define PGPU_CAT(a, b) PGPU_CAT2(a, b)

namespace pgpu {

int PGPU_CAT(launch_startree_scan_fx_mode, PGPU_MODE)(const KStarParams& p, size_t lds_bytes, void* stream) {
  const int grid = p.num_wgs;
  if (grid <= 0 || p.num_segs <= 0) return 0;
  hipLaunchKernelGGL(startree_scan_fx_kernel<PGPU_MODE>, dim3(grid), dim3(StarBlock<PGPU_MODE>::value), lds_bytes,
                     reinterpret_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pgpu
