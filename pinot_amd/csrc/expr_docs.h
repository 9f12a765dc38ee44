// expr_docs.h -- the device's doc loop of an expression program, shared by the two kernels that evaluate one per doc and
// look the result's key up in a sorted key array: expr_leaf_bitmap_kernel (kernels.hip: WHERE price * qty > 1000) and
// derive_ids_kernel (k_derive.hip: GROUP BY a + b).  The scan's expression instances have their own (device.h
// expr_batch: they read operands through the segment records at matched docs).
#pragma once
#include "device.h"

namespace pgpu {

// kU 64-doc steps of one wave at once, lane `lane` taking doc base + u * 64 + lane of step u (base is wave-uniform):
// live[u] <- the doc exists (< num_docs), out[u] <- the program's double over the doc's operands, 0.0 operands for a
// doc that does not.  A wave's 64 docs read adjacent forward-index words of each operand.  The chain dictId -> double
// is two dependent loads per operand and a step on its own waits for both, so the dictIds of every operand and step are
// gathered first, then the doubles, and only then is the program interpreted (expr_eval over a register stack).  Lanes
// past num_docs load nothing.  A template over the operands' and the program's types: a caller reads its task through
// the constant address space (cmem<ExprOperands>) or as a kernel argument, and either way they stay scalar operands.
template <int kU, typename Ops, typename Prog>
__device__ __forceinline__ void expr_eval_docs(const Ops& ops, const Prog& prog, int64_t base, int lane, int32_t num_docs,
                                               bool (&live)[kU], double (&out)[kU]) {
  const int nc = prog.ncols;
  uint32_t id[kExprMaxCols][kU];
  double v[kExprMaxCols][kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) live[u] = base + u * 64 + lane < num_docs;
#pragma unroll
  for (int c = 0; c < kExprMaxCols; ++c) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      id[c][u] = 0;
      v[c][u] = 0.0;
    }
    if (c < nc) {  // wave-uniform
#pragma unroll
      for (int u = 0; u < kU; ++u)
        if (live[u]) id[c][u] = gather_id(ops.fwd[c], ops.bits[c], base + u * 64 + lane);
    }
  }
#pragma unroll
  for (int c = 0; c < kExprMaxCols; ++c)
    if (c < nc) {
#pragma unroll
      for (int u = 0; u < kU; ++u)
        if (live[u]) v[c][u] = gp(ops.dval[c])[id[c][u]];
    }
  expr_eval<kU>(prog, v, out);
}

// The index of the first of the n ascending keys set[0, n) that is >= key (n: there is none).
__device__ __forceinline__ int key_lower_bound(gmem<int64_t>* __restrict__ set, int n, int64_t key) {
  int a = 0, b = n;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (set[mid] < key) a = mid + 1;
    else b = mid;
  }
  return a;
}

}  // namespace pgpu
