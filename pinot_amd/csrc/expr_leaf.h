// expr_leaf.h -- host side of the expression filter leaves (WHERE price * qty > 1000): the task one leaf of one segment
// hands to expr_leaf_bitmap_kernel and the job list of a plan's tasks.  Plain host code over internal.h's structs, so
// the planner (rt_plan_create.cpp), the launch (rt_exec.cpp) and tools/expr_filter_check.cpp share it.
#pragma once
#include <string.h>

#include <vector>

#include "internal.h"

namespace pgpu {

// The task of a leaf whose translated predicate is `raw` -- inclusive key bounds {lo, hi} (in == false) or sorted
// distinct keys (in == true), translate_raw_predicate's forms -- over program `prog` with operands `ops` (expr_operands,
// expr_eval.h) of a segment of num_docs docs, writing the docbits region at word `dst`.  The keys of an IN leaf are
// appended to *vals, whose first free index is vals_base + vals->size() in the plan's key array.
inline KExprLeafTask make_expr_leaf_task(const ExprProg& prog, const ExprOperands& ops, int32_t num_docs, bool in,
                                         const std::vector<int64_t>& raw, int negate, int64_t dst, int64_t vals_base,
                                         std::vector<int64_t>* vals) {
  KExprLeafTask t;
  memset(&t, 0, sizeof t);
  t.ops = ops;
  t.prog = prog;
  t.dst = dst;
  t.num_docs = num_docs;
  t.negate = negate ? 1 : 0;
  if (in) {
    t.kind = LEAF_RAW_IN;
    t.lo = vals_base + (int64_t)vals->size();
    t.hi = (int64_t)raw.size();
    vals->insert(vals->end(), raw.begin(), raw.end());
  } else {
    t.kind = LEAF_RAW_RANGE;
    t.lo = raw.size() > 0 ? raw[0] : 1;  // (no bounds: the empty range)
    t.hi = raw.size() > 1 ? raw[1] : 0;
  }
  return t;
}

// The kernel's work items: kExprLeafJobDocs docs of one task each, every doc of every task covered once.
inline void expr_leaf_jobs(const std::vector<KExprLeafTask>& tasks, std::vector<KExprLeafJob>* jobs) {
  jobs->clear();
  for (size_t i = 0; i < tasks.size(); ++i)
    for (int64_t d = 0; d < tasks[i].num_docs; d += kExprLeafJobDocs) jobs->push_back(KExprLeafJob{(int32_t)i, (int32_t)d});
}

// Docbits words a leaf's region takes for a segment of num_docs docs (emit_raw_task's rule: padded to an even count).
inline int64_t leaf_region_words(int64_t num_docs) { return (((num_docs + 31) / 32) + 1) & ~int64_t(1); }

}  // namespace pgpu
