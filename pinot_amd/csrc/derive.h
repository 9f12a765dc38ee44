// derive.h -- what the host (rt_dict.cpp ensure_derived) and the kernels of k_derive.hip share: the task of building one
// derived column -- the dictionary column of a group-by expression in one pinned segment (GROUP BY a + b).
//   candidates  the program over the mixed-radix product of the operands' segment-local dictionaries (operand 0 the
//               fastest digit) -> expr_value_key per combination; the host sorts and uniques them (group_expr.h)
//   ids         per doc: the operands' dictIds, their doubles, the program, the key's index in the sorted candidates ->
//               4 bytes per doc of scratch; the candidate is marked used
//   pack        remap[scratch[doc]] (candidate -> local dictId, the used candidates compacted on the host) as Pinot's
//               MSB-first fixed-bit forward index in pgpu_pin_segment's padded layout
#pragma once
#include <stdint.h>

#include "expr_eval.h"

namespace pgpu {

struct KDeriveTask {
  ExprOperands ops;            // (expr_eval.h; dval: ensure_values)
  int32_t card[kExprMaxCols];  // the operands' segment-local dictionary sizes (>= 1)
  ExprProg prog;               // (col[] is not read on the device)
  int32_t num_docs;
  int32_t pad;
};
static_assert(__builtin_offsetof(KDeriveTask, prog) == 96 && sizeof(KDeriveTask) == 320, "the layout the kernels were built for");

constexpr int kDeriveBlockDocs = 8192;  // docs per workgroup of the ids and the pack kernel: one forward-index tile

// keys[p] <- the key of combination p, p < product (the product of T.card[0 .. ncols)).
int launch_derive_candidates(const KDeriveTask& T, int64_t product, int64_t* keys, void* stream);
// scratch[doc] <- the index of the doc's key in cand[0, ncand) (sorted, unique), used[that index] <- 1, doc < T.num_docs.
int launch_derive_ids(const KDeriveTask& T, const int64_t* cand, int32_t ncand, uint32_t* scratch, uint32_t* used,
                      void* stream);
// fwd[0, fwd_words) <- the forward index of remap[scratch[doc]] at `bits` per doc, docs past num_docs and the padding 0;
// fwd_words = ceil(num_docs / 8192) * 256 * bits + 4.
int launch_derive_pack(const uint32_t* scratch, const int32_t* remap, int32_t num_docs, int32_t bits, uint32_t* fwd,
                       int64_t fwd_words, void* stream);

}  // namespace pgpu
