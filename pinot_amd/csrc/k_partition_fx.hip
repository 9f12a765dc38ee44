// k_partition_fx.hip -- the FX instances of the partitioned group-by's aggregate kernels (partition.h K8d / K8h), for
// plans with fixed-point FLOAT / DOUBLE sums (agreed plans of PGPU_OPT_EXACT_FP_SUM): the record passes K8a / K8c / K8e
// carry the operand's double as one stream, and these kernels split it into its W digits (fx_sum.h) where the records
// are accumulated.  An object of its own, so the kernels of k_partition.hip keep their code.
#define PGPU_PARTITION_FX 1
#include "partition.h"

namespace pgpu {

int launch_part_aggregate_fx(const KPartParamsFx& pp, size_t lds_bytes, void* stream) {
  hipLaunchKernelGGL(part_aggregate_fx_kernel, dim3(pp.num_parts), dim3(kBlock), lds_bytes,
                     reinterpret_cast<hipStream_t>(stream), pp);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_part_hash_aggregate_fx(const KPartParamsFx& pp, size_t lds_bytes, void* stream) {
  hipLaunchKernelGGL(part_hash_aggregate_fx_kernel, dim3(pp.num_parts), dim3(kBlock), lds_bytes,
                     reinterpret_cast<hipStream_t>(stream), pp);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pgpu
