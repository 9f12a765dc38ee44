// k_direct.hip — the direct-load scan kernel's instances of one family in one accumulator mode: compiled with
// -DPGPU_FAMILY=0|1|2|3|4 (ScanFamily: base, FX, DC, HIST, EXPR) and -DPGPU_MODE=0|1|2 (LDS, GLOBAL, HASH).  Which instances those
// are, and their template arguments, is kScanInstances' to say (internal.h).
#include <utility>

#include "scan_direct.h"

#if !defined(PGPU_MODE) || !defined(PGPU_FAMILY)
#error "compile with -DPGPU_FAMILY=0 (base), 1 (FX), 2 (DC), 3 (HIST) or 4 (EXPR) and -DPGPU_MODE=0 (LDS), 1 (GLOBAL) or 2 (HASH)"
#endif
#if (PGPU_FAMILY == 2 || PGPU_FAMILY == 3) && PGPU_MODE == 2
#error "the DC and HIST instances exist for MODE_LDS and MODE_GLOBAL only"
#endif

namespace pgpu {

// The kernel of row V, or null where the row is of another family or mode (a row not taken instantiates nothing).
template <int V>
static const void* instance() {
  constexpr ScanInstance I = kScanInstances[V];
  if constexpr (I.family != PGPU_FAMILY || !(I.modes >> PGPU_MODE & 1))
    return nullptr;
  else if constexpr (I.family == SCAN_FX)
    return reinterpret_cast<const void*>(filter_groupby_fx_kernel<PGPU_MODE, I.dense>);
  else if constexpr (I.family == SCAN_DC)
    return reinterpret_cast<const void*>(filter_groupby_dc_kernel<PGPU_MODE, I.dense>);
  else if constexpr (I.family == SCAN_HIST)
    return reinterpret_cast<const void*>(filter_groupby_hist_kernel<PGPU_MODE, I.dense>);
  else if constexpr (I.family == SCAN_EXPR)
    return reinterpret_cast<const void*>(filter_groupby_expr_kernel<PGPU_MODE, I.dense>);
  else
    return reinterpret_cast<const void*>(
        filter_groupby_kernel<PGPU_MODE, I.dense, I.simple, I.pair, I.fast, I.lane_batch>);
}

template <int... V>
static const void* instance_of(int variant, std::integer_sequence<int, V...>) {
  // (last row first: the kernels are laid out in the code object in the order they are named here, and this is the
  // order they have always had)
  static const void* const kernels[] = {instance<kScanVariants - 1 - V>()...};
  return kernels[kScanVariants - 1 - variant];
}

// variant: in [0, kScanVariants) (scan_entry checks it).
KernelEntry PGPU_OBJECT_ENTRY(scan, PGPU_FAMILY, PGPU_MODE)(ScanVariant variant) {
  return {instance_of(variant, std::make_integer_sequence<int, kScanVariants>{}), kBlock};
}

}  // namespace pgpu
