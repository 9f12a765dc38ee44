// k_startree.hip — the star-tree document scan of one accumulator mode: compiled with -DPGPU_MODE=0|1|2 and
// -DPGPU_FAMILY=0 (the plain instance) or 1 (the one for plans with fixed-point FLOAT / DOUBLE sums, SLOT_SUM_FX
// slots).  The traversal (mode-independent) lives in the plain mode-0 object.
#if PGPU_FAMILY != 0
#define PGPU_STAR_SCAN_ONLY 1
#endif
#include "startree_kernels.h"

#if !defined(PGPU_MODE) || !defined(PGPU_FAMILY)
#error "compile with -DPGPU_FAMILY=0 (plain) or 1 (FX) and -DPGPU_MODE=0 (LDS), 1 (GLOBAL) or 2 (HASH)"
#endif

namespace pgpu {

KernelEntry PGPU_OBJECT_ENTRY(star, PGPU_FAMILY, PGPU_MODE)() {
#if PGPU_FAMILY == 0
  return {reinterpret_cast<const void*>(startree_scan_kernel<PGPU_MODE>), StarBlock<PGPU_MODE>::value};
#else
  return {reinterpret_cast<const void*>(startree_scan_fx_kernel<PGPU_MODE>), StarBlock<PGPU_MODE>::value};
#endif
}

#if PGPU_MODE == 0 && PGPU_FAMILY == 0
int launch_startree_traverse(const KStarSeg* segs, int32_t num_segs, int64_t* seg_total, uint64_t deadline,
                             unsigned long long* stats, void* stream) {
  if (num_segs <= 0) return 0;
  hipLaunchKernelGGL(startree_traverse_kernel, dim3(num_segs), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     segs, seg_total, deadline, stats);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif

}  // namespace pgpu
