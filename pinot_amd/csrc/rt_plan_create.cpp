// rt_plan_create.cpp -- plan_create_impl: a query over a segment list becomes a plan, in named phases that share one
// PlanCtx (rt.h; the predicate translation and the sizing helpers the phases call are rt_plan.cpp's).
#include "expr_leaf.h"
#include "rt_decls.h"

namespace pgpu {
namespace {

// What the phases of one plan_create_impl call share beyond the plan itself; each is set by the phase named.
struct PlanCtx {
  pgpu_table_s* t;
  const pgpu_query* q;
  pgpu_plan_s* P;
  const StreamExec* se;
  int64_t G = 1;   // group-key space (layout_keys)
  int nslots = 0;  // accumulator slots (choose_table_mode)
  bool any_raw_leaf = false;                  // bind_query_columns
  std::vector<int64_t> gcard;                 // build_device_arrays: the global dictionary sizes of the key columns
  std::vector<ParsedPred> parsed;             // prepare_translation, as the flags and the two qcol vectors below
  std::vector<std::vector<int>> star_comps;
  bool star_allowed = false, exempt_kind = false, minmax_kind = false, any_star = false, any_inv = false;
  std::vector<int> qcol_key;   // per query column: its group-by key index (-1: none)
  std::vector<char> qcol_val;  // ... and whether an accumulator reads its values
  std::vector<int> qcol_dc;    // ... and its DISTINCTCOUNT entry (pgpu_plan_s::dc; -1: none)
  std::vector<int> qcol_hist;  // ... and its histogram (pgpu_plan_s::hist; -1: none)
  std::vector<int> perm;       // order_leaves: evaluation position -> predicate
  // per predicate, used by the REGEXP_LIKE ones: the DFA (bind_query_columns), the snapshot taken under the table
  // mutex (plan_regex_leaves) and the LEAF_SET words per plan segment, computed on the device (run_regex_leaves)
  std::vector<RegexJob> regex;
  double t_start = 0, tr[8] = {0};  // trace marks
  int ntr = 0;
  void mark() { if (trace_on() && ntr < 8) tr[ntr++] = now_us(); }
};

// One contiguous run of segments, translated: records carry chunk-relative tile / set offsets, fixed up when the
// chunks are concatenated in segment order (merge_chunk).
struct Chunk {
  bool gathers = false;  // pgpu_plan_s::gathers
  std::vector<uint8_t> rec;
  std::vector<uint32_t> set_words;
  std::vector<std::pair<int64_t, int64_t>> set_fix;
  std::vector<std::pair<int64_t, int64_t>> bit_fix;
  std::vector<KBitTask> bit_tasks;
  std::vector<KBitBlock> bit_blocks;
  std::vector<KRawTask> raw_tasks;
  std::vector<int64_t> raw_vals;
  std::vector<KExprLeafTask> expr_tasks;
  std::vector<int64_t> expr_vals;
  std::vector<std::shared_ptr<InvIndex>> inv_refs;
  std::vector<pgpu_plan_s::GenericStat> generic;  // rec: chunk-relative record index
  bool any_leap2 = false;
  int64_t docbit_words = 0;
  std::vector<uint8_t> scanned;
  int64_t tiles = 0, entries = 0, matched = 0, sel_docs = 0, exempt = 0;
  int64_t leaf_kinds[kLeafKinds] = {};
  int64_t sketch_leaves[2] = {};  // pgpu_plan_s::sketch_leaves
  double sel = 1.0;
  int rc = 0;
  std::string err;
};

// The query column (KCol index) of table column `col`, added on first use.
int query_col(pgpu_plan_s* P, int col) {
  for (size_t i = 0; i < P->query_cols.size(); ++i)
    if (P->query_cols[i] == col) return (int)i;
  P->query_cols.push_back(col);
  return (int)P->query_cols.size() - 1;
}

// The column of predicate l in segment s.  An expression leaf (a predicate on a virtual column) has none: a plain
// dictionary column without any index stands in, so the leaf is nobody's sorted, inverted or range-index leaf.
const Column& pred_column(const pgpu_plan_s* P, const Segment* s, const pgpu_query* q, int l) {
  static const Column kNoColumn;
  return P->expr_leaf(l) ? kNoColumn : s->cols[q->predicates[l].column];
}

// True for a REGEXP_LIKE predicate (a LIKE arrives as one): RegexpLikePredicate.  Its leaf is always a scan over the
// forward index -- without an FST index FilterOperatorUtils.getLeafFilterOperator (:65-72) takes a
// ScanBasedFilterOperator whatever other index the column has -- and its evaluator is never always-true or
// always-false (BaseDictionaryBasedPredicateEvaluator.java:26-41), so the leaf is never folded.
bool regex_leaf(const pgpu_query* q, int l) { return q->predicates[l].type == PGPU_PRED_REGEXP_LIKE; }

// Segment references (SegmentDataManager acquire): the table mutex is held only to take them here and, in
// build_device_arrays, to build the lazily made LUT / value arrays and snapshot the global dictionary sizes -- the
// per-segment translation runs unlocked, so concurrent queries on one table plan in parallel.
int acquire_segments(PlanCtx& cx, const int64_t* handles, int32_t nsegs) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  P->refs = std::make_shared<PlanRefs>();
  std::lock_guard<std::mutex> g(t->mu);
  P->segs.reserve(nsegs);
  P->refs->segs.reserve(nsegs);
  for (int i = 0; i < nsegs; ++i) {
    const int64_t h = handles[i];
    const std::shared_ptr<Segment>* sp = h > 0 && h < (int64_t)t->by_handle.size() ? &t->by_handle[h] : nullptr;
    if (!sp || !*sp) return fail(PGPU_ERR_NOT_FOUND, "unknown segment handle %lld", (long long)h);
    P->segs.push_back(sp->get());
    P->refs->segs.push_back(*sp);
  }
  return 0;
}

// The program of the table's virtual column vcol (an expression), copied under the table mutex (registrations append to
// the table's list); `what` prefixes the message for a column that is none.
int table_expr_prog(pgpu_table_s* t, int vcol, const char* what, ExprProg* out) {
  std::lock_guard<std::mutex> g(t->mu);
  const int e = vcol - (int)t->names.size();
  if (e < 0 || e >= (int)t->exprs.size()) return fail(PGPU_ERR_INVALID_ARGUMENT, "%s: bad column %d", what, vcol);
  *out = t->exprs[e].prog;
  return 0;
}

// Predicate i is on the virtual column vcol (ExpressionFilterOperator): its program, admitted over every planned
// segment (check_expr_segment).  Operands are those of expression aggregations: dictionary columns (STRING and virtual
// operands were refused when the expression was registered).
int bind_expr_leaf(PlanCtx& cx, int i, int vcol) {
  ExprProg& prog = cx.P->leaf_exprs[i];
  const std::string what = "predicate " + std::to_string(i);
  TRY(table_expr_prog(cx.t, vcol, what.c_str(), &prog));
  for (const Segment* s : cx.P->segs) TRY(check_expr_segment(cx.t, *s, prog, false, (what + ": expression").c_str()));
  cx.any_raw_leaf = true;  // planned and launched as a raw-value leaf is: a docbits region per query
  return 0;
}

// Group-by i names the group expression gcol (pgpu_table_add_group_expression): every planned segment gets its derived
// column now (under the table mutex; built on the GPU where this is its first use, ensure_derived), before anything
// reads a key column's cardinality.  Declined here: an external table, as for the other plans that are not a plain
// table of real columns; the cross-GPU entry points check pgpu_plan_s::group_exprs.
int bind_group_expr(PlanCtx& cx, int i, int gcol) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  if (cx.se && cx.se->d_table) return fail(PGPU_ERR_UNSUPPORTED, "a GROUP BY expression with an external table");
  std::lock_guard<std::mutex> g(t->mu);
  if (!t->has_dict_col(gcol)) return fail(PGPU_ERR_INVALID_ARGUMENT, "group-by %d: bad column %d", i, gcol);
  for (Segment* s : P->segs) TRY(ensure_derived(t, *s, gcol, t->stream));
  const ExprProg& prog = t->gexprs[gcol - kGroupExprBase].prog;
  P->group_exprs.push_back({gcol, std::vector<int32_t>(prog.col, prog.col + prog.ncols)});
  return 0;
}

// Predicate and group-by columns become query columns.  Raw (no-dictionary) columns: aggregation operands and
// raw-value predicate leaves; a group-by on one runs on Pinot's NoDictionary*GroupKeyGenerator, not here.
int bind_query_columns(PlanCtx& cx) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  const int ncols = (int)cx.t->names.size();
  for (int i = 0; i < q->num_predicates; ++i) {  // REGEXP_LIKE: declined here, before anything is built for the plan
    if (!regex_leaf(q, i)) continue;
    const pgpu_predicate& pr = q->predicates[i];
    if (pr.num_values != 1 || !pr.values || !pr.values[0])
      return fail(PGPU_ERR_INVALID_ARGUMENT, "REGEXP_LIKE predicate %d takes one value, the pattern", i);
    TRY(regex_check_column(cx.t, P->segs, pr.column));
    if (cx.regex.empty()) cx.regex.resize(q->num_predicates);
    TRY(regex_compile_pattern(pr.values[0], &cx.regex[i].dfa));  // the one compilation of the plan
  }
  for (int i = 0; i < q->num_predicates; ++i)
    if (q->predicates[i].column >= ncols) { P->leaf_exprs.assign(q->num_predicates, ExprProg{}); break; }
  for (int i = 0; i < q->num_predicates; ++i) {
    const int c = q->predicates[i].column;
    if (c >= ncols) {  // a virtual column: the operands are read by the leaf's own kernel, not by the scan -- the
      TRY(bind_expr_leaf(cx, i, c));  // leaf's record column (never read: a LEAF_BITMAP) is its first operand
      P->leaf_slot.push_back(query_col(P, P->leaf_exprs[i].col[0]));
      continue;
    }
    if (c < 0) return fail(PGPU_ERR_INVALID_ARGUMENT, "predicate %d: bad column %d", i, c);
    P->leaf_slot.push_back(query_col(P, c));
  }
  P->num_leaves = q->num_predicates;
  for (int i = 0; i < q->num_group_by; ++i) {
    const int c = q->group_by[i];
    if (is_group_expr_col(c)) {  // a group-by expression: from here on the dictionary column Segment::col(c) resolves
      TRY(bind_group_expr(cx, i, c));
    } else if (c < 0 || c >= ncols) {
      return fail(PGPU_ERR_INVALID_ARGUMENT, "group-by %d: bad column %d", i, c);
    }
    P->key_cols.push_back(c);
    query_col(P, c);
  }
  for (Segment* s : P->segs) {
    for (int i = 0; i < q->num_predicates; ++i) {
      if (P->expr_leaf(i)) continue;
      const Column& c = s->cols[q->predicates[i].column];
      cx.any_raw_leaf |= c.raw;
      if (c.raw && cx.t->types[q->predicates[i].column] == PGPU_STRING)
        return fail(PGPU_ERR_UNSUPPORTED, "predicate on raw STRING column %d", q->predicates[i].column);
    }
    for (int i = 0; i < q->num_group_by; ++i)
      if (s->col(q->group_by[i]).raw)
        return fail(PGPU_ERR_UNSUPPORTED, "group-by on raw (no-dictionary) column %d", q->group_by[i]);
  }
  return 0;
}

// The filter program, a function of the query alone: the postfix ops, whether it is one AND over every predicate in
// order (or a single leaf), and the evaluation stack's depth.
int compile_filter(const pgpu_query* q, std::vector<int32_t>* ops, bool* pure_and_out, int* max_depth_out) {
  int depth = 0, max_depth = 0;
  bool pure_and = q->num_filter_ops > 0;
  int leaves_seen = 0;
  for (int i = 0; i < q->num_filter_ops; ++i) {
    const pgpu_filter_op& o = q->filter[i];
    if (o.op == PGPU_OP_PRED) {
      if (o.arg < 0 || o.arg >= q->num_predicates) return fail(PGPU_ERR_INVALID_ARGUMENT, "bad predicate index");
      if (o.arg != leaves_seen) pure_and = false;
      ++leaves_seen;
      ++depth;
      ops->push_back((OP_LEAF << 16) | o.arg);
    } else if (o.op == PGPU_OP_NOT) {
      if (depth < 1) return fail(PGPU_ERR_INVALID_ARGUMENT, "malformed filter program");
      pure_and = false;
      ops->push_back(OP_NOT << 16);
    } else if (o.op == PGPU_OP_AND || o.op == PGPU_OP_OR) {
      if (o.arg < 1 || o.arg > depth) return fail(PGPU_ERR_INVALID_ARGUMENT, "malformed filter program");
      if (o.op == PGPU_OP_OR || i != q->num_filter_ops - 1) pure_and = false;
      depth -= o.arg - 1;
      ops->push_back(((o.op == PGPU_OP_AND ? OP_AND : OP_OR) << 16) | o.arg);
    } else {
      return fail(PGPU_ERR_INVALID_ARGUMENT, "bad filter opcode %d", o.op);
    }
    max_depth = std::max(max_depth, depth);
  }
  if (q->num_filter_ops > 0 && depth != 1) return fail(PGPU_ERR_INVALID_ARGUMENT, "malformed filter program");
  if (max_depth > kMaxStack) return fail(PGPU_ERR_UNSUPPORTED, "filter nesting deeper than %d", kMaxStack);
  if (q->num_filter_ops == 1) pure_and = true;  // a single leaf
  if (pure_and && leaves_seen != q->num_predicates) pure_and = false;
  *pure_and_out = pure_and;
  *max_depth_out = max_depth;
  return 0;
}

// One accumulator slot: its kind, its table column (-1: none, the COUNT), its fixed-point digit (-1: none) and format.
void push_slot(pgpu_plan_s* P, int kind, int tcol, int fx_digit, const FxFormat& fmt) {
  P->slot_kind.push_back(kind);
  P->slot_tcol.push_back(tcol);
  // (a slot of an expression reads its program's operand columns, bound by add_expr_slot: no query column of its own)
  P->slot_col.push_back(tcol == -1 || is_expr_tcol(tcol) ? 0 : query_col(P, tcol));
  P->slot_expr.push_back(-1);
  P->slot_fx.push_back(fx_digit);
  P->slot_fmt.push_back(fmt);
  P->slot_dc.push_back(-1);
  P->slot_pct.push_back(-1);
}

// The slot of (kind, tcol), shared by the aggregations that need the same one.
int add_slot(pgpu_plan_s* P, int kind, int tcol) {
  for (size_t s = 1; s < P->slot_kind.size(); ++s)
    if (P->slot_kind[s] == kind && P->slot_tcol[s] == tcol && P->slot_fx[s] < 0 && !P->side_slot(s)) return (int)s;
  push_slot(P, kind, tcol, -1, FxFormat{});
  return (int)P->slot_kind.size() - 1;
}

// The row of DISTINCTCOUNT(tcol), shared by the aggregations of the column: an ordinary row of the group table that
// starts at 0 and that the scan never touches -- SLOT_SUM_I64 to everything but the DC scan instances (rt.h dc).
int add_distinct_slot(pgpu_plan_s* P, int tcol) {
  for (const pgpu_plan_s::Distinct& d : P->dc)
    if (d.tcol == tcol) return d.slot;
  push_slot(P, SLOT_SUM_I64, tcol, -1, FxFormat{});
  pgpu_plan_s::Distinct d;
  d.slot = (int32_t)P->slot_kind.size() - 1;
  d.tcol = tcol;
  d.qcol = P->slot_col[d.slot];
  P->slot_dc[d.slot] = (int32_t)P->dc.size();
  P->dc.push_back(d);
  return d.slot;
}

// The histogram of table column tcol in a plan with PERCENTILE aggregations, shared by everything that reads the column.
int add_hist(pgpu_plan_s* P, int tcol) {
  for (size_t h = 0; h < P->hist.size(); ++h)
    if (P->hist[h].tcol == tcol) return (int)h;
  pgpu_plan_s::Hist h;
  h.tcol = tcol;
  h.qcol = query_col(P, tcol);
  P->hist.push_back(h);
  return (int)P->hist.size() - 1;
}

// The row of one PERCENTILE aggregation (its own: two percentiles of a column are two rows over one histogram): an
// ordinary row of the group table that starts at 0 and that the scan never touches -- SLOT_SUM_F64 to everything but
// the histogram scan instances (rt.h pct).
int add_percentile_slot(pgpu_plan_s* P, int tcol, int32_t p_e4) {
  push_slot(P, SLOT_SUM_F64, tcol, -1, FxFormat{});
  pgpu_plan_s::Percentile e;
  e.slot = (int32_t)P->slot_kind.size() - 1;
  e.hist = add_hist(P, tcol);
  e.p_e4 = p_e4;
  P->slot_pct[e.slot] = (int32_t)P->pct.size();
  P->pct.push_back(e);
  return e.slot;
}

// The plan's entry of the table's virtual column vcol (an expression), added on first use with its operand columns as
// query columns (*out), once it is admitted over every planned segment (check_expr_segment).
int plan_expr(PlanCtx& cx, int vcol, int* out) {
  pgpu_plan_s* P = cx.P;
  for (size_t e = 0; e < P->exprs.size(); ++e)
    if (P->exprs[e].vcol == vcol) { *out = (int)e; return 0; }
  pgpu_plan_s::PlanExpr pe;
  pe.vcol = vcol;
  TRY(table_expr_prog(cx.t, vcol, "aggregation", &pe.prog));
  if ((int)P->exprs.size() >= kMaxPlanExprs)
    return fail(PGPU_ERR_UNSUPPORTED, "more than %d distinct expression aggregations in one query", kMaxPlanExprs);
  for (const Segment* s : P->segs) TRY(check_expr_segment(cx.t, *s, pe.prog, false, "expression"));
  for (int c = 0; c < pe.prog.ncols; ++c) query_col(P, pe.prog.col[c]);
  P->exprs.push_back(pe);
  *out = (int)P->exprs.size() - 1;
  return 0;
}

// The slot of (kind, expression e): SUM and AVG share the float64 sum, MIN and MAX have a key row each.
int add_expr_slot(pgpu_plan_s* P, int kind, int e) {
  const int s = add_slot(P, kind, expr_tcol(e));
  P->slot_expr[s] = e;
  return s;
}

// The W digit slots of a fixed-point sum: adjacent, of the one column, shared by SUM and AVG of the column.
int add_fx_slots(pgpu_plan_s* P, int tcol, const FxFormat& f) {
  for (size_t s = 1; s < P->slot_kind.size(); ++s)
    if (P->slot_fx[s] == 0 && P->slot_tcol[s] == tcol) return (int)s;
  // SLOT_SUM_I64: what the digit's word is after the scan's accumulate (rt.h slot_fx)
  for (int j = 0; j < f.W; ++j) push_slot(P, SLOT_SUM_I64, tcol, j, f);
  P->fx = true;
  return (int)P->slot_kind.size() - f.W;
}

// The segments that decide a sum's slot: the plan's own, or those of every part of a composite plan with fixed-point
// sums (fx_scope), so the parts' slots line up.
const std::vector<Segment*>& sum_scope(const pgpu_plan_s* P) { return P->fx_scope.empty() ? P->segs : P->fx_scope; }

// PGPU_OPT_EXACT_FP_SUM: the fixed-point format of aggregation i, a SUM / AVG over a.column (fx_sum.h) -- E and L over
// every operand the plan can read (the segments' dictionaries or raw docs, and the pre-aggregated doubles of the
// star-trees that may answer the query), the headroom from the docs of the same segments; an agreed plan takes the
// agreed range and the docs of every rank instead (FxAgree).  Mode 0 when an operand is not finite: the sum keeps its
// float64 slot.
FxFormat fx_format_for(const PlanCtx& cx, int i) {
  const pgpu_plan_s* P = cx.P;
  int64_t docs = 0;
  FxRange r;
  if (P->fx_agreed) {
    const FxAgree& g = P->fx_ranges[i];
    r.E = g.E;
    r.L = g.L;
    r.any = g.any != 0;
    r.finite = g.finite != 0;
    docs = g.docs;
  } else {
    r = fx_operand_range(cx.t, sum_scope(P), cx.q, cx.q->aggs[i].column, &docs);
  }
  return fx_format(r, docs);
}

// The slot (the first of the digit slots) of aggregation i over a numeric column.
int agg_slot_for(PlanCtx& cx, int i, int* slot) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  const pgpu_agg& a = q->aggs[i];
  const int type = cx.t->types[a.column];
  int kind;
  switch (PGPU_AGG_FN(a.fn)) {
    case PGPU_AGG_SUM: case PGPU_AGG_AVG: {
      // Integer columns sum exactly in int64 unless the plan could overflow it: |sum| <= sum over segments of
      // numDocs x max |value| (the sorted dictionary's ends).  Past 2^62 the slot accumulates the doubles of
      // the values (Pinot's own arithmetic, SumAggregationFunction.java:66-73) instead of wrapping.
      // (an agreed plan: the bound summed over every rank's segments, so every rank has the same slots)
      const bool fits = is_int_type(type) && (P->fx_agreed ? P->fx_ranges[i].int_sum_bound < 0x1p62
                                                           : int_sum_fits(sum_scope(P), a.column));
      kind = fits ? SLOT_SUM_I64 : SLOT_SUM_F64;
      break;
    }
    case PGPU_AGG_MIN: kind = SLOT_MIN_KEY; break;
    case PGPU_AGG_MAX: kind = SLOT_MAX_KEY; break;
    default: return fail(PGPU_ERR_UNSUPPORTED, "aggregation function %d", a.fn);
  }
  if (kind == SLOT_SUM_F64 && (q->options & PGPU_OPT_EXACT_FP_SUM)) {
    const FxFormat f = fx_format_for(cx, i);
    if (f.mode != FX_NONE) {
      *slot = add_fx_slots(P, a.column, f);
      return 0;
    }
  }
  *slot = add_slot(P, kind, a.column);
  return 0;
}

// Aggregations -> accumulator slots (slot 0 = COUNT), the hidden docId slot, and what fixed-point sums change in the
// plan's configuration.
int assign_slots(PlanCtx& cx) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  const int ncols = (int)cx.t->names.size();
  push_slot(P, SLOT_COUNT, -1, -1, FxFormat{});
  if (P->fx_agreed) {
    if (!(q->options & PGPU_OPT_EXACT_FP_SUM)) return fail(PGPU_ERR_INVALID_ARGUMENT, "agreed ranges without PGPU_OPT_EXACT_FP_SUM");
    if ((int)P->fx_ranges.size() != q->num_aggs) return fail(PGPU_ERR_INVALID_ARGUMENT, "one agreed range per aggregation");
    for (int i = 0; i < q->num_aggs; ++i)
      if ((P->fx_ranges[i].is_sum != 0) != (q->aggs[i].fn == PGPU_AGG_SUM || q->aggs[i].fn == PGPU_AGG_AVG))
        return fail(PGPU_ERR_INVALID_ARGUMENT, "aggregation %d: the agreed range is not of this aggregation", i);
  }
  for (int i = 0; i < q->num_aggs; ++i) {
    const pgpu_agg& a = q->aggs[i];
    // the function code (bits 0..7; a PERCENTILE carries its percentile above them, codes 0..5 nothing)
    const int fn = PGPU_AGG_FN(a.fn);
    if (fn != PGPU_AGG_PERCENTILE && a.fn != fn) return fail(PGPU_ERR_UNSUPPORTED, "aggregation function %d", a.fn);
    P->agg_fn.push_back(fn);
    P->agg_col.push_back(a.column);
    if (fn == PGPU_AGG_COUNT) {  // (COUNT never reads its argument, but the column must be one: the results name it)
      if (a.column >= ncols) {
        std::lock_guard<std::mutex> g(cx.t->mu);
        if (a.column - ncols >= (int)cx.t->exprs.size())
          return fail(PGPU_ERR_INVALID_ARGUMENT, "aggregation %d: bad column", i);
      }
      P->agg_slot.push_back(0);
      continue;
    }
    if (a.column >= ncols) {  // a virtual column: an expression over real columns (pgpu_table_add_expression)
      if (fn == PGPU_AGG_DISTINCTCOUNT || fn == PGPU_AGG_PERCENTILE)
        return fail(PGPU_ERR_UNSUPPORTED, "%s of an expression (virtual column %d)",
                    fn == PGPU_AGG_PERCENTILE ? "PERCENTILE" : "DISTINCTCOUNT", a.column);
      if (fn != PGPU_AGG_SUM && fn != PGPU_AGG_AVG && fn != PGPU_AGG_MIN && fn != PGPU_AGG_MAX)
        return fail(PGPU_ERR_UNSUPPORTED, "aggregation function %d", a.fn);
      if (q->options & PGPU_OPT_EXACT_FP_SUM)
        return fail(PGPU_ERR_UNSUPPORTED, "an expression aggregation with PGPU_OPT_EXACT_FP_SUM");
      int e = 0;
      TRY(plan_expr(cx, a.column, &e));
      P->agg_slot.push_back(add_expr_slot(P, fn == PGPU_AGG_MIN   ? SLOT_MIN_KEY
                                             : fn == PGPU_AGG_MAX ? SLOT_MAX_KEY
                                                                  : SLOT_SUM_F64, e));
      continue;
    }
    if (a.column < 0 || a.column >= ncols) return fail(PGPU_ERR_INVALID_ARGUMENT, "aggregation %d: bad column", i);
    if (fn == PGPU_AGG_PERCENTILE) {
      const int32_t p_e4 = PGPU_AGG_PERCENTILE_E4(a.fn);
      if (p_e4 > PGPU_AGG_PERCENTILE_MAX_E4)
        return fail(PGPU_ERR_INVALID_ARGUMENT, "aggregation %d: PERCENTILE of %d ten-thousandths, above 100", i, p_e4);
      if (q->options & PGPU_OPT_EXACT_FP_SUM)
        return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE with PGPU_OPT_EXACT_FP_SUM");
      if (cx.t->types[a.column] == PGPU_STRING)
        return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE over STRING column %d", a.column);
      for (const Segment* s : P->segs)
        if (s->cols[a.column].raw)
          return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE over raw (no-dictionary) column %d", a.column);
      P->agg_slot.push_back(add_percentile_slot(P, a.column, p_e4));
      continue;
    }
    if (fn == PGPU_AGG_DISTINCTCOUNT) {  // any column type: the set is over dictIds
      if (q->options & PGPU_OPT_EXACT_FP_SUM)
        return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT with PGPU_OPT_EXACT_FP_SUM");
      for (const Segment* s : P->segs)
        if (s->cols[a.column].raw)
          return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT over raw (no-dictionary) column %d", a.column);
      P->agg_slot.push_back(add_distinct_slot(P, a.column));
      continue;
    }
    if (cx.t->types[a.column] == PGPU_STRING) return fail(PGPU_ERR_UNSUPPORTED, "numeric aggregation over a STRING column");
    int slot = 0;
    TRY(agg_slot_for(cx, i, &slot));
    P->agg_slot.push_back(slot);
  }
  // hidden MIN($docId): each group's first matching doc (its IntGroupIdMap id order)
  if (P->first_doc_slot) push_slot(P, SLOT_MIN_KEY, kDocIdColumn, -1, FxFormat{});
  if (P->fx) {
    // A streamed plan configures before its later chunks are planned: a plan with fixed-point sums runs as one launch.
    // A plain one takes the scan kernel's global / hash tables (pinned by the tests of the option as it shipped); an
    // agreed one keeps the partitioned pipelines, whose record passes carry the operand's double as one stream and
    // whose aggregate kernels split it (K8d / K8h FX, partition.h).
    if (!P->fx_agreed) {
      P->cfg.partitioned_group_by = 0;
      P->cfg.hash_partitions = 0;
    }
    P->cfg.stream_chunks = 1;
  }
  if (!P->dc.empty()) {
    // as a plain plan with fixed-point sums: the scan kernel's LDS / global tables, one launch
    if ((int)P->dc.size() > kMaxDistinct)
      return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT over more than %d columns in one query", kMaxDistinct);
    if (P->first_doc_slot) return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT in a numGroupsLimit (composite) plan");
    P->cfg.partitioned_group_by = 0;
    P->cfg.hash_partitions = 0;
    P->cfg.stream_chunks = 1;
  }
  if (!P->pct.empty()) {
    // histograms only: the plan's DISTINCTCOUNT columns are counted from one too (the non-zero cells of a row)
    for (const pgpu_plan_s::Distinct& d : P->dc) P->hist[add_hist(P, d.tcol)].dc_slot = d.slot;
    if ((int)P->hist.size() > kMaxDistinct)
      return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE: more than %d side columns (histograms) in one query", kMaxDistinct);
    if (P->first_doc_slot) return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE in a numGroupsLimit (composite) plan");
    long double docs = 0;
    for (const Segment* s : P->segs) docs += (long double)s->num_docs;
    if (docs >= 4294967296.0L)
      return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE over segments of 2^32 docs or more (a histogram cell could wrap)");
    P->cfg.partitioned_group_by = 0;
    P->cfg.hash_partitions = 0;
    P->cfg.stream_chunks = 1;
  }
  if (!P->exprs.empty()) {
    // the scan's expression instance: its own family, so not beside the side structures of another; one launch on the
    // scan kernel's own tables (LDS, global, hash), never the partitioned pipelines
    if (!P->dc.empty() || !P->pct.empty())
      return fail(PGPU_ERR_UNSUPPORTED, "an expression aggregation in one query with %s",
                  !P->pct.empty() ? "PERCENTILE" : "DISTINCTCOUNT");
    if (P->first_doc_slot) return fail(PGPU_ERR_UNSUPPORTED, "an expression aggregation in a numGroupsLimit (composite) plan");
    if (cx.se && cx.se->d_table) return fail(PGPU_ERR_UNSUPPORTED, "an expression aggregation with an external table");
    P->cfg.partitioned_group_by = 0;
    P->cfg.hash_partitions = 0;
    P->cfg.stream_chunks = 1;
  }
  if ((int)P->slot_kind.size() > kMaxSlots) return fail(PGPU_ERR_UNSUPPORTED, "too many accumulators");
  if ((int)P->query_cols.size() > kMaxQueryCols) return fail(PGPU_ERR_UNSUPPORTED, "too many columns");
  // TransformOperator.getNumColumnsProjected: distinct group-by and aggregation columns -- for an expression the
  // columns it names (AggregationOperator.java:90 counts the projection's columns, each once)
  // (a group-by expression projects its operands; its derived column is no column of the reference's segment)
  std::vector<int> proj;
  for (int c : P->key_cols)
    if (!is_group_expr_col(c)) proj.push_back(c);
  for (const pgpu_plan_s::GroupExprRef& ge : P->group_exprs) proj.insert(proj.end(), ge.operands.begin(), ge.operands.end());
  for (int i = 0; i < q->num_aggs; ++i) {
    if (q->aggs[i].column >= ncols) {  // (a COUNT never reads its argument: of an expression it projects nothing)
      for (const pgpu_plan_s::PlanExpr& pe : P->exprs)
        if (pe.vcol == q->aggs[i].column) proj.insert(proj.end(), pe.prog.col, pe.prog.col + pe.prog.ncols);
      continue;
    }
    if (q->aggs[i].column >= 0) proj.push_back(q->aggs[i].column);
  }
  std::sort(proj.begin(), proj.end());
  P->num_projected = (int)(std::unique(proj.begin(), proj.end()) - proj.begin());
  return 0;
}

// numGroupsLimit: the plan is sensitive to it when some segment's local key space exceeds it.
void note_groups_limit(PlanCtx& cx) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  P->num_groups_limit = q->num_groups_limit;
  P->pql_cap = !(q->options & PGPU_OPT_SQL_GROUP_BY);
  if (q->num_groups_limit <= 0) return;
  for (Segment* s : P->segs) {
    int64_t prod = 1;
    for (int c : P->key_cols) {
      const int64_t card = std::max<int64_t>(s->col(c).card, 1);
      prod = prod > INT64_MAX / card ? INT64_MAX : prod * card;
    }
    if (prod > q->num_groups_limit) P->limit_sensitive = true;
  }
}

// This segment's column keeps its local value arrays (the table-global ones take the rest, ensure_value_map).
bool keeps_local_values(const pgpu_table_s* t, int c, const Column& col) {
  return col.raw || col.card < kGlobalValuesMinCard || (is_int_type(t->types[c]) && col.key_affine);
}

// (under the table mutex) the key LUTs, the value arrays and the docId index of every segment.
int plan_segment_arrays(PlanCtx& cx) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  const hipStream_t stream = t->stream;
  const size_t nk = P->key_cols.size();
  const size_t nd = P->dc.size(), nh = P->hist.size();
  P->key_lut.resize(P->segs.size() * nk);
  P->dc_lut.resize(P->segs.size() * nd);
  P->hist_lut.resize(P->segs.size() * nh);
  P->refs->luts.reserve(P->segs.size() * (nk + nd + nh));
  for (size_t i = 0; i < P->segs.size(); ++i) {
    Segment* s = P->segs[i];
    for (size_t j = 0; j < nk; ++j) {
      const int c = P->key_cols[j];
      TRY(ensure_lut(t, *s, c, stream));
      const Column& col = s->col(c);
      P->refs->luts.push_back(col.lut);
      KeyLut& kl = P->key_lut[i * nk + j];
      kl.lut = col.lut_off >= 0 ? nullptr : reinterpret_cast<const int32_t*>(col.lut->p);
      kl.off = col.lut_off;
    }
    std::vector<int32_t> vcols;
    for (size_t k = 1; k < P->slot_kind.size(); ++k) {
      if (P->side_slot(k)) continue;
      P->slot_value_cols(k, &vcols);  // the slot's column, or the operands of its expression
      for (int32_t c : vcols) TRY(ensure_values(t, *s, c, stream));
    }
    for (const ExprProg& g : P->leaf_exprs)  // expression leaves: their operands' dictId -> double tables
      for (int c = 0; c < g.ncols; ++c) TRY(ensure_values(t, *s, g.col[c], stream));
    if (P->first_doc_slot) TRY(ensure_docid(t, s->num_docs, stream));
  }
  // the distinct columns' local -> global mapping, as a key column's (after the key LUTs: plan_star_segment indexes
  // refs->luts by segment and key)
  for (size_t i = 0; i < P->segs.size(); ++i)
    for (size_t d = 0; d < nd; ++d) {
      const int c = P->dc[d].tcol;
      TRY(ensure_lut(t, *P->segs[i], c, stream));
      const Column& col = P->segs[i]->cols[c];
      P->refs->luts.push_back(col.lut);
      KeyLut& kl = P->dc_lut[i * nd + d];
      kl.lut = col.lut_off >= 0 ? nullptr : reinterpret_cast<const int32_t*>(col.lut->p);
      kl.off = col.lut_off;
    }
  // ... and the histogram columns' (of the same snapshot where a column has both)
  for (size_t i = 0; i < P->segs.size(); ++i)
    for (size_t h = 0; h < nh; ++h) {
      const int c = P->hist[h].tcol;
      TRY(ensure_lut(t, *P->segs[i], c, stream));
      const Column& col = P->segs[i]->cols[c];
      P->refs->luts.push_back(col.lut);
      KeyLut& kl = P->hist_lut[i * nh + h];
      kl.lut = col.lut_off >= 0 ? nullptr : reinterpret_cast<const int32_t*>(col.lut->p);
      kl.off = col.lut_off;
    }
  return 0;
}

// (under the table mutex) the values percentile_select_kernel reads: each histogram column's snapshot of the global
// dictionary as doubles -- (double)value of an INT / LONG column (PercentileAggregationFunction reads
// getDoubleValuesSV), the value of a FLOAT / DOUBLE one.  A column that only a DISTINCTCOUNT reads has none.
int plan_hist_values(PlanCtx& cx) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  for (size_t h = 0; h < P->hist.size(); ++h) {
    pgpu_plan_s::Hist& H = P->hist[h];
    bool wanted = false;
    for (const pgpu_plan_s::Percentile& e : P->pct) wanted |= e.hist == (int32_t)h;
    if (!wanted) continue;
    std::vector<double> v((size_t)H.card, 0.0);
    if (is_int_type(H.dict->type))
      for (size_t i = 0; i < H.dict->iv.size(); ++i) v[i] = (double)H.dict->iv[i];
    else
      for (size_t i = 0; i < H.dict->dv.size(); ++i) v[i] = H.dict->dv[i];
    auto m = std::make_shared<DevMem>();
    HIP_TRY(hipMalloc(&m->p, sizeof(double) * v.size()));
    HIP_TRY(hipMemcpyAsync(m->p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    H.values = std::move(m);
  }
  return 0;
}

// (under the table mutex) accumulator columns whose values are gathered (FLOAT / DOUBLE, or integers not
// consecutive): the table-global arrays where a segment's dictionary maps onto the global one.
int plan_global_values(PlanCtx& cx) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  P->val_cols.clear();
  std::vector<int32_t> slot_cols, cols;
  for (size_t k = 1; k < P->slot_kind.size(); ++k) {
    if (P->side_slot(k)) continue;  // a DISTINCTCOUNT / PERCENTILE row reads no values in the scan
    P->slot_value_cols(k, &slot_cols);  // (the hidden docId slot: none)
    cols.insert(cols.end(), slot_cols.begin(), slot_cols.end());
  }
  for (const int c : cols) {
    if (std::find(P->val_cols.begin(), P->val_cols.end(), c) != P->val_cols.end()) continue;
    bool any = false;
    for (Segment* s : P->segs) {
      const Column& col = s->cols[c];
      if (keeps_local_values(t, c, col)) continue;
      TRY(ensure_value_map(t, *s, c));
      any |= col.vgap_first >= 0;
    }
    if (any) {
      TRY(ensure_global_values(t, c, t->stream));
      P->val_cols.push_back(c);
    }
  }
  P->val_map.assign(P->segs.size() * P->val_cols.size(), ValMap{});
  for (size_t v = 0; v < P->val_cols.size(); ++v) {
    const int c = P->val_cols[v];
    const auto& gv = t->gvalues[c];
    P->refs->luts.push_back(gv.keys);
    P->refs->luts.push_back(gv.vals);
    for (size_t i = 0; i < P->segs.size(); ++i) {
      const Column& col = P->segs[i]->cols[c];
      ValMap& vm = P->val_map[i * P->val_cols.size() + v];
      if (keeps_local_values(t, c, col) || col.vmap_version != t->global_version[c] || col.vgap_first < 0) continue;
      vm.keys = reinterpret_cast<const int64_t*>(gv.keys->p) + col.vgap_first;
      vm.vals = reinterpret_cast<const double*>(gv.vals->p) + col.vgap_first;
      vm.ngaps = (int32_t)col.vgaps.size();
      std::copy(col.vgaps.begin(), col.vgaps.end(), vm.gaps.begin());
    }
  }
  return 0;
}

// (under the table mutex) REGEXP_LIKE leaves: the column's dictionary on the device and the planned segments' LUTs, of
// the snapshot the rest of the plan is built on (rt_regex.cpp).  Only references are taken here.
int plan_regex_leaves(PlanCtx& cx) {
  const pgpu_query* q = cx.q;
  for (int l = 0; l < q->num_predicates; ++l)
    if (regex_leaf(q, l)) TRY(regex_job_snapshot(cx.t, cx.P->segs, q->predicates[l].column, &cx.regex[l]));
  return 0;
}

// (the table mutex released) The DFA over the global dictionary and every planned segment's local bitset, on the
// device: planners of other queries on the table are not kept waiting for the round trip.
int run_regex_leaves(PlanCtx& cx) {
  pgpu_plan_s* P = cx.P;
  for (int l = 0; l < cx.q->num_predicates; ++l) {
    if (!regex_leaf(cx.q, l)) continue;
    RegexJob& job = cx.regex[l];
    TRY(regex_job_run(cx.t, &job, nullptr));
    P->regex_stats[0] += (int64_t)job.tasks.size();
    P->regex_stats[1] += job.affine;
    P->regex_stats[2] += job.dict_bytes;
    P->regex_stats[3] += job.dfa.table_bytes();
  }
  return 0;
}

// Under the table mutex: the global dictionary sizes the key layout is built on, and every segment's device LUT /
// value arrays of the referenced columns (built once per segment, rebuilt out of place when the global dictionary
// grows) -- taken together, so the LUTs the plan points at map into exactly the key space it sizes.
int build_device_arrays(PlanCtx& cx) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  const size_t nk = P->key_cols.size();
  cx.gcard.resize(nk);
  std::lock_guard<std::mutex> table_lock(t->mu);
  P->key_dicts.resize(nk);
  for (size_t j = 0; j < nk; ++j) {
    P->key_dicts[j] = t->col_global(P->key_cols[j]);
    cx.gcard[j] = (int64_t)P->key_dicts[j]->size();
  }
  for (pgpu_plan_s::Distinct& d : P->dc) {  // the bitmap's width: the snapshot the LUTs taken below map into
    d.dict = t->global[d.tcol];
    d.card = std::max<int64_t>((int64_t)d.dict->size(), 1);
    d.words = (d.card + 63) / 64;
  }
  for (pgpu_plan_s::Hist& h : P->hist) {  // the histogram's width, likewise
    h.dict = t->global[h.tcol];
    h.card = std::max<int64_t>((int64_t)h.dict->size(), 1);
    h.stride = (h.card + 3) & ~int64_t(3);
  }
  TRY(plan_segment_arrays(cx));
  TRY(plan_global_values(cx));
  TRY(plan_hist_values(cx));
  TRY(plan_regex_leaves(cx));
  P->docid_fwd = t->d_docid_fwd;
  P->docid_key = t->d_docid_key;
  P->docid_bits = t->docid_bits;
  return 0;
}

// The global ids [*a, *b) of dictionary gd that an EQ / IN / RANGE predicate admits.
void admitted_ids(const Dict& gd, const pgpu_predicate& pr, const ParsedPred& pp, int64_t* a, int64_t* b) {
  auto search = [&](const Literal& v) {
    return is_int_type(gd.type) ? sorted_search<int64_t>(gd.iv, v.i) : sorted_search<double>(gd.dv, v.d);
  };
  if (pr.type == PGPU_PRED_RANGE) {  // as translate_predicate_dict's RANGE, on the global dictionary
    if (pp.lits[0].star) *a = 0;
    else { const int ins = search(pp.lits[0]); *a = ins < 0 ? -(ins + 1) : (pr.lower_inclusive ? ins : ins + 1); }
    if (pp.lits[1].star) *b = (int64_t)gd.size();
    else { const int ins = search(pp.lits[1]); *b = ins < 0 ? -(ins + 1) : (pr.upper_inclusive ? ins + 1 : ins); }
    return;
  }
  *a = INT64_MAX;
  *b = INT64_MIN;
  for (const Literal& v : pp.lits) {
    const int ins = search(v);
    if (ins >= 0) { *a = std::min<int64_t>(*a, ins); *b = std::max<int64_t>(*b, ins + 1); }
  }
  if (*a > *b) *a = *b = 0;
}

// Key space restricted by the filter: a group-by column that a top-level conjunct of the filter bounds (EQ / IN /
// RANGE on the same numeric column) can only produce the global ids inside that bound -- C3's GROUP BY
// daysSinceEpoch under "daysSinceEpoch BETWEEN 17849 AND 17856" has 8 possible keys, not 365.  Column j's key
// digit becomes (global id - key_off[j]); the kernels subtract key_bias = sum key_off[j] * stride[j] once.  Same
// groups, a table (and slab fold, and compaction) sized by what the filter admits.  *kspan: the digits' spans.
int restrict_key_space(PlanCtx& cx, std::vector<int64_t>* kspan_out) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  std::vector<int64_t> klo(P->key_cols.size(), 0), kspan(cx.gcard);
  if (P->pure_and) {
    for (size_t j = 0; j < P->key_cols.size(); ++j) {
      const int c = P->key_cols[j];
      const Dict& gd = *P->key_dicts[j];
      if (!is_int_type(gd.type) && !is_fp_type(gd.type)) continue;
      int64_t lo = 0, hi = (int64_t)gd.size();
      for (int l = 0; l < q->num_predicates; ++l) {
        const pgpu_predicate& pr = q->predicates[l];
        if (pr.column != c || (pr.type != PGPU_PRED_EQ && pr.type != PGPU_PRED_IN && pr.type != PGPU_PRED_RANGE)) continue;
        ParsedPred pp;
        TRY(parse_predicate(cx.t->col_type(c), pr, &pp));
        int64_t a = 0, b = 0;
        admitted_ids(gd, pr, pp, &a, &b);
        lo = std::max(lo, a);
        hi = std::min(hi, b);
      }
      if (hi <= lo) { lo = 0; hi = 1; }  // nothing admitted: no doc can match, keep a one-key digit
      klo[j] = lo;
      kspan[j] = hi - lo;
    }
    int64_t prod = 1;  // ARRAY_MAP stage plans keep the full key space (their stages restart the strides)
    bool ovf = false;
    for (size_t j = 0; j < P->key_cols.size(); ++j) {
      const int64_t card = std::max<int64_t>(kspan[j], 1);
      if (prod > INT64_MAX / card) ovf = true;
      else prod *= card;
    }
    if (ovf) { std::fill(klo.begin(), klo.end(), 0); kspan = cx.gcard; }
  }
  P->key_off = klo;
  *kspan_out = std::move(kspan);
  return 0;
}

// ArrayMapBasedHolder (DictionaryBasedGroupKeyGenerator.java:127-137: the cardinality product overflows a long).
// The key columns split into consecutive groups whose keys fit 62 bits: group s's key (the previous group's slot x
// its own key space + the mixed-radix key of its columns) is mapped on the device to its slot in hash table s --
// a dense id below 2^31 -- and the last group's key is the group key of the plan's hash table.  Exact, like the
// IntArray map it replaces; the tables are decoded back to dictIds at finalize.
int stage_array_map_keys(pgpu_plan_s* P) {
  const int nk = (int)P->key_cols.size();
  constexpr int64_t kLim = INT64_C(1) << 62;
  int64_t docs = 0;
  for (Segment* s : P->segs) docs += s->num_docs;
  std::vector<int> ends;
  std::vector<int64_t> spaces, caps;
  int64_t capp = 1;  // slots of the previous group's table (1: none)
  for (int j = 0; j < nk;) {
    int64_t l = 1;
    int k = j;
    while (k < nk && l <= kLim / capp / P->key_card[k]) l *= P->key_card[k++];
    if (k == j) return fail(PGPU_ERR_UNSUPPORTED, "group key space beyond the staged ARRAY_MAP keys");
    for (int i = j; i < k; ++i)  // strides restart within each group
      P->key_stride[i] = i == j ? 1 : P->key_stride[i - 1] * P->key_card[i - 1];
    ends.push_back(k);
    spaces.push_back(l);
    if (k == nk) break;
    const int64_t want = std::max<int64_t>(2 * std::min<int64_t>(capp * l, std::max<int64_t>(docs, 1)), 1024);
    int64_t cap = 1;
    while (cap < want) cap <<= 1;
    if (cap > (INT64_C(1) << 31)) return fail(PGPU_ERR_UNSUPPORTED, "ARRAY_MAP key stage beyond 2^31 slots");
    caps.push_back(cap);
    capp = cap;
    j = k;
  }
  P->stage_end.assign(ends.begin(), ends.end() - 1);
  P->stage_cap = caps;
  P->stage_space = spaces;  // per group (the last one included)
  P->stage_mult.assign(spaces.begin() + 1, spaces.end());
  return 0;
}

// Group-key layout over the table-global dictionaries (mixed radix, first column fastest: ArrayBasedHolder), staged
// when the product overflows.
int layout_keys(PlanCtx& cx, const std::vector<int64_t>& kspan) {
  pgpu_plan_s* P = cx.P;
  bool overflow = false;
  int64_t G = 1;
  for (size_t j = 0; j < P->key_cols.size(); ++j) {
    const int64_t card = std::max<int64_t>(kspan[j], 1);
    P->key_card.push_back(card);
    P->key_stride.push_back(G);
    if (!overflow && G > INT64_MAX / card) overflow = true;
    else if (!overflow) G *= card;
  }
  P->key_bias = 0;
  if (!overflow)
    for (size_t j = 0; j < P->key_cols.size(); ++j) P->key_bias += P->key_off[j] * P->key_stride[j];
  if (overflow) {
    TRY(stage_array_map_keys(P));
    G = INT64_C(1) << 40;  // beyond every dense table: the hash table (no overflow in the sizing products)
  }
  cx.G = G;
  return 0;
}

// LDS, GLOBAL or HASH table, and the hash table's size.
void choose_table_mode(PlanCtx& cx) {
  pgpu_table_s* t = cx.t;
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  const int64_t G = cx.G;
  const int nslots = cx.nslots = (int)P->slot_kind.size();
  constexpr int64_t kDenseGlobalMax = int64_t(1) << 26;
  // LDS-privatised tables up to 112 KB (one workgroup per CU at the top end): measured on MI355X, an 80 KB table
  // (C4: 5000 groups x 2 slots) runs 2.1x faster in LDS than with global atomics.  pgpu_config.lds_table_kb.
  const int64_t kLdsBudget = (int64_t)std::max(1, P->cfg.lds_table_kb) * 1024;
  // direct kernel LDS: [table (MODE_LDS)] [filter stack (general programs)] [per-wave match queues] (scan_lds_layout,
  // the kernel's own; reserve_leap2 adds the STATS_LEAP2 bytes)
  const size_t stack_bytes = (size_t)scan_lds_layout(0, P->pure_and).maps;
  for (Segment* s : P->segs) P->total_docs += s->num_docs;
  P->pack_slot = lds_pack_slot(t, P, q, G);
  const int lds_rows = nslots - (P->pack_slot >= 0 ? 1 : 0);
  if ((int64_t)lds_rows * G * 8 <= kLdsBudget) {
    P->mode = MODE_LDS;
    P->num_keys = G;
    P->lds_bytes = (size_t)scan_lds_layout((int64_t)lds_rows * G, P->pure_and).maps;
  } else if (G <= kDenseGlobalMax) {
    P->pack_slot = -1;
    P->mode = MODE_GLOBAL;
    P->num_keys = G;
    P->lds_bytes = stack_bytes;
  } else {
    P->mode = MODE_HASH;
    P->hash = true;
    P->pack_slot = hash_pack_slot(t, P, q, &P->pack_shift);
    // Groups are bounded by the key space and, per segment, by min(its local key space, its docs): C5-style keys of
    // small per-segment cardinalities need far fewer slots than 2 x docs.  A cached plan re-sizes from the group
    // count its last execution found (hash_capacity, plan_cache_get): same query, same segments, same groups.
    int64_t bound = 0;
    for (Segment* s : P->segs) {
      int64_t local = 1;
      for (int c : P->key_cols) {
        const int64_t card = std::max<int64_t>(s->col(c).card, 1);
        local = local > (int64_t)s->num_docs / card ? (int64_t)s->num_docs + 1 : local * card;
      }
      bound += std::min<int64_t>(local, s->num_docs);
    }
    P->group_bound = std::max<int64_t>(1, std::min<int64_t>(G, bound));
    P->groups_seen = std::make_shared<std::atomic<int64_t>>(-1);
    P->num_keys = hash_capacity(P->group_bound);
    P->lds_bytes = stack_bytes;
  }
}

// DISTINCTCOUNT plans: dense key spaces only (the bitmap rows are indexed by the composite key), and side bitmaps of at
// most kDistinctMaxBytes in all.
int check_distinct_shape(const PlanCtx& cx) {
  const pgpu_plan_s* P = cx.P;
  if (!P->pct.empty()) {  // histograms only (those of the plan's DISTINCTCOUNT columns among them)
    if (P->mode == MODE_HASH)
      return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE over a key space that takes the hash table (%s)",
                  P->stage_end.empty() ? "past 2^26 keys" : "ARRAY_MAP stages");
    long double bytes = 0;
    for (const pgpu_plan_s::Hist& h : P->hist) bytes += (long double)P->num_keys * (long double)h.stride * 4.0L;
    if (bytes > (long double)kDistinctMaxBytes)
      return fail(PGPU_ERR_UNSUPPORTED, "PERCENTILE histograms of %.0Lf bytes (%lld keys), above the cap of %lld", bytes,
                  (long long)P->num_keys, (long long)kDistinctMaxBytes);
    return 0;
  }
  if (P->dc.empty()) return 0;
  if (P->mode == MODE_HASH)
    return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT over a key space that takes the hash table (%s)",
                P->stage_end.empty() ? "past 2^26 keys" : "ARRAY_MAP stages");
  long double bytes = 0;
  for (const pgpu_plan_s::Distinct& d : P->dc) bytes += (long double)P->num_keys * (long double)d.words * 8.0L;
  if (bytes > (long double)kDistinctMaxBytes)
    return fail(PGPU_ERR_UNSUPPORTED, "DISTINCTCOUNT bitmaps of %.0Lf bytes (%lld keys), above the cap of %lld", bytes,
                (long long)P->num_keys, (long long)kDistinctMaxBytes);
  return 0;
}

// What the per-segment translation reads besides the plan: the record stride, the parsed literals, the star-tree
// composites, which aggregation-only answers skip the post-filter scan, and the roles of the query columns.
int prepare_translation(PlanCtx& cx) {
  pgpu_table_s* t = cx.t;
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  const int nqc = (int)P->query_cols.size();
  P->seg_scanned.reserve(P->segs.size());
  P->seg_stride = (int)(sizeof(KSegHdr) + sizeof(KCol) * nqc + sizeof(KLeaf) * std::max(P->num_leaves, 0));
  P->seg_stride = (P->seg_stride + 15) & ~15;
  P->segrec.reserve(P->segs.size() * (size_t)P->seg_stride);
  cx.parsed.resize(P->num_leaves);
  for (int l = 0; l < P->num_leaves; ++l)
    // (an expression's value is a DOUBLE: its literals are read by Double.parseDouble)
    TRY(parse_predicate(P->expr_leaf(l) ? PGPU_DOUBLE : t->types[q->predicates[l].column], q->predicates[l], &cx.parsed[l]));
  // (DISTINCTCOUNT: StarTreeUtils finds no function-column pair for it -- such a plan scans)
  cx.star_allowed = q->num_group_by > 0 && !(q->options & PGPU_OPT_NO_STAR_TREE) && P->stage_end.empty() &&
                    P->dc.empty() && P->pct.empty() && P->exprs.empty() && star_composites(P->ops, q, &cx.star_comps);
  // (a filter with an expression leaf never takes the star-tree: StarTreeUtils.java:255-258)
  // (nor does one with a REGEXP_LIKE: StarTreeUtils.java:266-274)
  for (int l = 0; l < P->num_leaves; ++l) cx.star_allowed &= !P->expr_leaf(l) && !regex_leaf(q, l);
  // Aggregation-only over a match-all segment: COUNT-only is answered from metadata, MIN / MAX / DISTINCTCOUNT-only
  // from the dictionaries (AggregationPlanNode.java:165-183, isFitForDictionaryBasedPlan :233-246; every dictionary
  // value occurs in its segment, so the scan gives the same set) -- same values, numEntriesScannedPostFilter 0
  // (MetadataBasedAggregationOperator.java:89-92, DictionaryBasedAggregationOperator.java:171-173).
  if (q->num_group_by == 0 && q->num_aggs > 0) {
    bool all_count = true, all_minmax = true;
    for (int i = 0; i < q->num_aggs; ++i) {
      // (a PERCENTILE is in neither: its unfiltered aggregation-only query scans -- fn carries upper bits besides)
      all_count &= q->aggs[i].fn == PGPU_AGG_COUNT;
      all_minmax &= q->aggs[i].fn == PGPU_AGG_MIN || q->aggs[i].fn == PGPU_AGG_MAX ||
                    q->aggs[i].fn == PGPU_AGG_DISTINCTCOUNT;
    }
    // (MIN / MAX of an expression: isFitForDictionaryBasedPlan wants an identifier as the argument -- it scans)
    if (!P->exprs.empty()) all_minmax = false;
    cx.exempt_kind = all_count || all_minmax;
    cx.minmax_kind = all_minmax && !all_count;
  }
  cx.mark();
  for (Segment* s : P->segs) {
    cx.any_star |= cx.star_allowed && s->star != nullptr;
    for (int l = 0; l < q->num_predicates; ++l)
      cx.any_inv |= pred_column(P, s, q, l).inv != nullptr;
  }
  cx.qcol_key.assign(P->query_cols.size(), -1);
  cx.qcol_val.assign(P->query_cols.size(), 0);
  for (size_t j = 0; j < P->key_cols.size(); ++j)
    for (size_t i = 0; i < P->query_cols.size(); ++i)
      if (P->query_cols[i] == P->key_cols[j]) cx.qcol_key[i] = (int)j;
  for (size_t k = 1; k < P->slot_col.size(); ++k)
    if (!P->side_slot(k) && P->slot_expr[k] < 0) cx.qcol_val[P->slot_col[k]] = 1;
  for (const pgpu_plan_s::PlanExpr& pe : P->exprs)  // the operands of the expressions: their doubles are gathered
    for (int c = 0; c < pe.prog.ncols; ++c) cx.qcol_val[query_col(P, pe.prog.col[c])] = 1;
  cx.qcol_dc.assign(P->query_cols.size(), -1);
  for (size_t d = 0; d < P->dc.size(); ++d) cx.qcol_dc[P->dc[d].qcol] = (int)d;
  cx.qcol_hist.assign(P->query_cols.size(), -1);
  for (size_t h = 0; h < P->hist.size(); ++h) cx.qcol_hist[P->hist[h].qcol] = (int)h;
  return 0;
}

// Pure-AND programs evaluate their leaves in order with a wave-uniform early exit (AndDocIdIterator); leaves on
// columns sorted in every segment go first (FilterOperatorUtils orders index-based children first,
// FilterOperatorUtils.java:143-178) -- their docId-range masks cost no memory traffic and let whole waves skip
// the scan leaves' bytes.
void order_leaves(PlanCtx& cx) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  std::vector<int>& perm = cx.perm;
  perm.resize(P->num_leaves);
  for (int l = 0; l < P->num_leaves; ++l) perm[l] = l;
  if (P->pure_and && P->num_leaves > 1) {
    // FilterOperatorUtils.reorderAndFilterChildOperators (:143-178): sorted-index leaves, then bitmap
    // (inverted-index) leaves, then range-index leaves, then scans.
    // ... then the expression leaves (ExpressionFilterOperator: priority 10, :171-172; the sort is stable).
    std::vector<int> first, second, third, rest, last;
    for (int l = 0; l < P->num_leaves; ++l) {
      const pgpu_predicate& pr = q->predicates[l];
      if (P->expr_leaf(l)) { last.push_back(l); continue; }
      if (regex_leaf(q, l)) { rest.push_back(l); continue; }  // a scan, whatever index the column has
      const bool eq_in = pr.type == PGPU_PRED_EQ || pr.type == PGPU_PRED_NOT_EQ || pr.type == PGPU_PRED_IN ||
                         pr.type == PGPU_PRED_NOT_IN;
      bool all_sorted = !P->segs.empty(), all_inv = !P->segs.empty() && eq_in && !P->no_inverted;
      bool all_rng = !P->segs.empty() && pr.type == PGPU_PRED_RANGE;
      for (Segment* s : P->segs) {
        all_sorted &= s->cols[pr.column].sorted;
        all_inv &= s->cols[pr.column].inv != nullptr && !s->star;
        all_rng &= s->cols[pr.column].rng != nullptr;
      }
      (all_sorted ? first : all_inv ? second : all_rng ? third : rest).push_back(l);
    }
    first.insert(first.end(), second.begin(), second.end());
    first.insert(first.end(), third.begin(), third.end());
    first.insert(first.end(), rest.begin(), rest.end());
    first.insert(first.end(), last.begin(), last.end());
    perm = first;
    std::vector<int32_t> slots(P->num_leaves);
    for (int k = 0; k < P->num_leaves; ++k) slots[k] = P->leaf_slot[perm[k]];
    P->leaf_slot = slots;
  }
  P->leaf_perm = perm;
}

// ------------------------------------------------------------------------------------ per-segment translation
// The predicates of segment s as leaves; returns the folded program's value over them.
int translate_leaves(const PlanCtx& cx, size_t seg_index, std::vector<LeafHost>& leaves, std::vector<Tri>& tri,
                     std::vector<int>& ids_scratch, Tri* whole) {
  const Segment* s = cx.P->segs[seg_index];
  const pgpu_query* q = cx.q;
  const pgpu_plan_s* P = cx.P;
  for (int l = 0; l < P->num_leaves; ++l) {
    LeafHost& lh = leaves[l];
    lh.kind = LEAF_NONE; lh.negate = 0; lh.lo = 0; lh.span = 0;
    const Column& pc = pred_column(P, s, q, l);
    if (P->expr_leaf(l)) {  // the raw DOUBLE evaluator over computed keys; never folded (ExpressionFilterOperator)
      translate_raw_predicate(PGPU_DOUBLE, q->predicates[l], cx.parsed[l], &lh);
      lh.kind = lh.kind == LEAF_RAW_IN ? LEAF_EXPR_IN : LEAF_EXPR_RANGE;
      tri[l] = T_VAR;
      continue;
    }
    if (regex_leaf(q, l)) {  // the device's bitset as it is: never folded, no index leaf, no sorted doc range
      lh.kind = LEAF_SET;
      lh.set = cx.regex[l].sets[seg_index];
      tri[l] = T_VAR;
      continue;
    }
    if (pc.raw) translate_raw_predicate(cx.t->types[q->predicates[l].column], q->predicates[l], cx.parsed[l], &lh);
    else TRY(translate_predicate(pc, q->predicates[l], cx.parsed[l], &lh, ids_scratch));
    if (!P->no_inverted && !s->star) to_inverted_leaf(pc, q->predicates[l], *s, &lh);
    tri[l] = leaves[l].kind == LEAF_NONE ? T_NONE : leaves[l].kind == LEAF_ALL ? T_ALL : T_VAR;
  }
  *whole = P->num_leaves ? fold_program(P->ops, tri) : T_ALL;
  return 0;
}

// DictionaryBasedAggregationOperator needs a dictionary on every MIN / MAX column (AggregationPlanNode.java:196-213)
bool raw_minmax(const PlanCtx& cx, const Segment* s) {
  if (!cx.minmax_kind) return false;
  for (int i = 0; i < cx.q->num_aggs; ++i)
    if (cx.q->aggs[i].column >= 0 && s->cols[cx.q->aggs[i].column].raw) return true;
  return false;
}

// numEntriesScannedInFilter (filter_stats.h): Pinot's leaf operators in this segment, its folded operator tree, and
// how the count is taken; returns the record's KSegHdr.stats.  The tree depends only on the leaves' operator kinds:
// classified once per distinct kind vector of the chunk (stat_cache; no per-segment allocation).
int32_t segment_stats(const PlanCtx& cx, const Segment* s, const std::vector<LeafHost>& leaves,
                      const std::vector<Tri>& tri, std::unordered_map<uint64_t, SegStats>& stat_cache, Chunk& C) {
  const pgpu_query* q = cx.q;
  const pgpu_plan_s* P = cx.P;
  uint64_t sig = 0;
  for (int l = 0; l < P->num_leaves; ++l) {
    const pgpu_predicate& pr = q->predicates[l];
    const Column& col = pred_column(P, s, q, l);
    // FilterOperatorUtils.getLeafFilterOperator (:42-82): sorted column -> SortedIndexBasedFilterOperator;
    // RANGE with a range index -> RangeIndexBasedFilterOperator; other predicates with an inverted index ->
    // BitmapBasedFilterOperator; else a scan.  An expression: ExpressionFilterOperator (FilterPlanNode.java:179-186)
    const int k = P->expr_leaf(l) ? SL_EXPR : regex_leaf(q, l) ? SL_SCAN : tri[l] == T_NONE ? SL_EMPTY : tri[l] == T_ALL ? SL_ALL : col.sorted ? SL_SORTED :
                  (pr.type != PGPU_PRED_RANGE && col.inv) ? SL_BITMAP :
                  (pr.type == PGPU_PRED_RANGE && col.rng && leaves[l].kind == LEAF_RANGE) ? SL_RANGEIDX : SL_SCAN;
    sig = sig * kStatLeafKinds + (uint64_t)k;
  }
  auto it = stat_cache.find(sig);
  if (it == stat_cache.end()) it = stat_cache.emplace(sig, classify_segment_stats(P, sig)).first;
  const SegStats& ss = it->second;
  C.any_leap2 |= (ss.rec_stats & 3) == KSTATS_LEAP2;
  if (ss.kind == STATS_CONST) C.entries += ss.const_per_doc * s->num_docs;
  for (int l : ss.range_leaves) {  // RangeIndexBasedFilterOperator's own partial-match scan
    const LeafHost& lh = leaves[l];
    C.entries += s->cols[q->predicates[l].column].rng->partial_entries(lh.lo, (int64_t)lh.lo + lh.span - 1);
  }
  if (ss.kind == STATS_GENERIC)
    C.generic.push_back({(int64_t)(C.rec.size() / P->seg_stride), s->num_docs, ss.tree, 0});
  return ss.rec_stats;
}

// The chunk's selectivity estimate, from the translated leaves of its first scanned segment.
void estimate_chunk_selectivity(const PlanCtx& cx, const Segment* s, const std::vector<LeafHost>& leaves, Chunk& C) {
  const pgpu_plan_s* P = cx.P;
  std::vector<double> frac(P->num_leaves, 1.0);
  for (int l = 0; l < P->num_leaves; ++l) {
    const LeafHost& lh = leaves[l];
    const double card = std::max(1, pred_column(P, s, cx.q, l).card);
    double f = lh.kind == LEAF_ALL ? 1.0 : lh.kind == LEAF_NONE ? 0.0 : lh.kind == LEAF_RANGE ? lh.span / card : 0.0;
    if (lh.kind == LEAF_DOCRANGE) f = (double)lh.span / std::max(1, s->num_docs);
    if (lh.kind == LEAF_BITMAP) f = lh.inv_frac;
    if (lh.kind == LEAF_RAW_RANGE || lh.kind == LEAF_RAW_IN) f = 0.5;  // no dictionary to estimate from
    if (lh.kind == LEAF_EXPR_RANGE || lh.kind == LEAF_EXPR_IN) f = 0.5;  // likewise
    if (regex_leaf(cx.q, l)) f = 0.5;  // likewise: the host does not look at the bits
    else if (lh.kind == LEAF_SET) {
      int64_t ones = 0;
      for (uint32_t w : lh.set) ones += __builtin_popcount(w);
      f = ones / card;
    }
    frac[l] = lh.negate ? 1.0 - f : f;
  }
  C.sel = P->num_leaves ? estimate_selectivity(P->ops, frac) : 1.0;
  C.sel_docs = s->num_docs;
}

// The record's KCol of every query column of segment i; true when one of them gathers (pgpu_plan_s::gathers).
bool fill_kcols(const PlanCtx& cx, size_t i, KCol* kc) {
  const pgpu_plan_s* P = cx.P;
  const Segment* s = P->segs[i];
  const int nqc = (int)P->query_cols.size();
  bool gathers = false;
  for (int j = 0; j < nqc; ++j) {
    const int tc = P->query_cols[j];
    const Column* c = tc == kDocIdColumn ? nullptr : &s->col(tc);
    if (!c || c->raw) {  // the virtual $docId, or values per doc: addressed through the identity docId index
      kc[j].fwd = P->docid_fwd;
      kc[j].lut = nullptr;
      kc[j].dkey = c ? c->d_key : P->docid_key;
      kc[j].dval = c ? c->d_val : nullptr;
      kc[j].bits = P->docid_bits;
    } else {
      kc[j].fwd = c->d_fwd;
      kc[j].bits = c->bits;
      if (cx.qcol_key[j] >= 0) {  // group-by key: the LUT version planned (the segment's current one may be newer)
        const KeyLut& kl = P->key_lut[i * P->key_cols.size() + cx.qcol_key[j]];
        kc[j].lut = kl.lut;
        kc[j].lut_off = kl.off;
      } else if (cx.qcol_dc[j] >= 0) {  // DISTINCTCOUNT column: the same mapping (of the same dictionary snapshot)
        const KeyLut& kl = P->dc_lut[i * P->dc.size() + cx.qcol_dc[j]];
        kc[j].lut = kl.lut;
        kc[j].lut_off = kl.off;
      } else if (cx.qcol_hist[j] >= 0) {  // histogram column: the same again
        const KeyLut& kl = P->hist_lut[i * P->hist.size() + cx.qcol_hist[j]];
        kc[j].lut = kl.lut;
        kc[j].lut_off = kl.off;
      }
      if (cx.qcol_val[j]) {  // accumulator operand: value arrays, built once (ensure_values) and never replaced
        kc[j].dkey = c->key_affine ? nullptr : c->d_key;
        kc[j].key_base = c->key_base;
        kc[j].dval = c->d_val;
        // or the table-global ones, as planned under the table mutex (ensure_value_map)
        for (size_t v = 0; v < P->val_cols.size(); ++v) {
          if (P->val_cols[v] != tc) continue;
          const ValMap& vm = P->val_map[i * P->val_cols.size() + v];
          if (vm.keys) {
            kc[j].dkey = vm.keys;
            kc[j].dval = vm.vals;
            kc[j].ngaps = vm.ngaps;
            std::copy(vm.gaps.begin(), vm.gaps.end(), kc[j].gaps);
          }
        }
      }
    }
    gathers |= ((cx.qcol_key[j] >= 0 || cx.qcol_dc[j] >= 0 || cx.qcol_hist[j] >= 0) && kc[j].lut != nullptr) ||
               (cx.qcol_val[j] && kc[j].dkey != nullptr);
  }
  return gathers || !P->exprs.empty();  // (an expression's operands are gathered per matched doc)
}

// LEAF_SET: the bitset words, every leaf's 8-byte aligned; `field`: the chunk offset of the record's KLeaf::set.
void emit_set_words(Chunk& C, const uint32_t* words, size_t n, int64_t field) {
  C.set_fix.emplace_back(field, (int64_t)C.set_words.size());
  C.set_words.insert(C.set_words.end(), words, words + n);
  if (C.set_words.size() & 1) C.set_words.push_back(0);
}

// A scan leaf as its column's byte-code sketch answers it (col_sketch.h): the code range of a LEAF_RANGE, the code set
// of a LEAF_SET.
struct SketchLeaf {
  bool on_sketched = false;  // a RANGE / SET leaf on a column that has a sketch
  bool exact = false;        // ... which the codes answer exactly
  bool use = false;          // ... and so do they every such leaf of the query on that column in this segment
  uint32_t lo = 0, span = 0;
  uint32_t codes[kSketchSetWords] = {};
};

// Which leaves of segment s read their column's sketch instead of its dictIds.  Called after everything that is
// decided from the dictId leaves (fold, index leaves, statistics, selectivity, instance): the swap changes the bytes
// a leaf reads and nothing else.  All-or-nothing per column: with one leaf left on the dictIds both copies would be
// read.  sk: per predicate; counts the pairs in C.sketch_leaves.
void choose_sketch_leaves(const PlanCtx& cx, const Segment* s, const std::vector<LeafHost>& leaves,
                          std::array<SketchLeaf, kMaxLeaves>& sk, Chunk& C) {
  const pgpu_plan_s* P = cx.P;
  const int nl = P->num_leaves;
  for (SketchLeaf& x : sk) x = SketchLeaf();
  if (!P->sketch_on || nl > kMaxLeaves) return;
  const Column* lcol[kMaxLeaves] = {};
  for (int l = 0; l < nl; ++l) {
    const LeafHost& lh = leaves[l];
    if ((lh.kind != LEAF_RANGE && lh.kind != LEAF_SET) || P->expr_leaf(l)) continue;
    const Column& col = pred_column(P, s, cx.q, l);
    if (!col.d_sketch || col.sketch.ncodes <= 0) continue;
    lcol[l] = &col;
    sk[l].on_sketched = true;
    if (lh.kind == LEAF_RANGE) {
      int a = 0, b = 0;
      sk[l].exact = sketch_range_exact(col.sketch, lh.lo, (int64_t)lh.lo + lh.span, &a, &b);
      sk[l].lo = (uint32_t)a;
      sk[l].span = (uint32_t)(b - a);
    } else {
      sk[l].exact = (int64_t)lh.set.size() * 32 >= col.card && sketch_set_exact(col.sketch, lh.set.data(), sk[l].codes);
    }
  }
  for (int l = 0; l < nl; ++l) {
    if (!sk[l].on_sketched) continue;
    bool all = true;
    for (int m = 0; m < nl; ++m)
      if (lcol[m] == lcol[l]) all &= sk[m].exact;
    sk[l].use = all;
    C.sketch_leaves[all ? 0 : 1]++;
  }
}

// Raw-value leaf: evaluated per query into a docId bitmap region (raw_leaf_bitmap_kernel, negation included) that the
// scan reads as a LEAF_BITMAP.
void emit_raw_task(Chunk& C, const Segment* s, const Column& col, const LeafHost& lh, KLeaf& kl, int64_t field) {
  C.bit_fix.emplace_back(field, C.docbit_words);
  KRawTask rt;
  memset(&rt, 0, sizeof rt);
  rt.keys = col.d_key;
  rt.dst = C.docbit_words;
  rt.num_docs = s->num_docs;
  rt.kind = lh.kind;
  rt.negate = lh.negate;
  if (lh.kind == LEAF_RAW_RANGE) {
    rt.lo = lh.raw[0];
    rt.hi = lh.raw[1];
  } else {
    rt.lo = (int64_t)C.raw_vals.size();
    rt.hi = (int64_t)lh.raw.size();
    C.raw_vals.insert(C.raw_vals.end(), lh.raw.begin(), lh.raw.end());
  }
  C.raw_tasks.push_back(rt);
  C.docbit_words += ((((int64_t)s->num_docs + 31) / 32) + 1) & ~int64_t(1);
  kl.kind = LEAF_BITMAP;
  kl.negate = 0;
}

// Expression leaf: evaluated per query into a docId bitmap region allocated by emit_raw_task's rule
// (expr_leaf_bitmap_kernel, negation included) that the scan reads as a LEAF_BITMAP.
void emit_expr_task(Chunk& C, const Segment* s, const ExprProg& prog, const LeafHost& lh, KLeaf& kl, int64_t field) {
  C.bit_fix.emplace_back(field, C.docbit_words);
  // (the operands' d_val: ensure_values, plan_segment_arrays)
  C.expr_tasks.push_back(make_expr_leaf_task(prog, expr_operands(*s, prog), s->num_docs, lh.kind == LEAF_EXPR_IN, lh.raw,
                                             lh.negate, C.docbit_words, 0, &C.expr_vals));
  C.docbit_words += leaf_region_words(s->num_docs);
  kl.kind = LEAF_BITMAP;
  kl.negate = 0;
}

// LEAF_BITMAP of one dictId (no OR to compute): the scan reads its containers in place through a block directory --
// BITMAP containers word by word, ARRAY containers (< 4096 docs of a block, e.g. a segment's partial last block) by a
// binary search of their sorted offsets (array_group_mask); entry = payload address, | 1 and the entry count in bits
// 48..63 for an ARRAY.  False (nothing emitted) when a container cannot be read so.
bool emit_bitdir(Chunk& C, const Segment* s, const Column& col, const LeafHost& lh, KLeaf& kl, int64_t field) {
  const InvIndex& inv = *col.inv;
  const InvIndex::Entry& e = inv.ids[lh.inv_ids[0]];
  auto payload = [&](const InvIndex::Cont& ct) {
    return reinterpret_cast<uint64_t>(reinterpret_cast<const uint32_t*>(inv.d_block) + ct.word);
  };
  for (int32_t ci = e.begin; ci < e.begin + e.count; ++ci) {
    const InvIndex::Cont& ct = inv.conts[ci];
    if (ct.type != CONT_BITMAP && !(ct.type == CONT_ARRAY && ct.n >= 0 && ct.n < 65536 && (payload(ct) >> 47) == 0))
      return false;
  }
  const int64_t nblk = ((int64_t)s->num_docs + 65535) >> 16;
  std::vector<uint64_t> dir((size_t)nblk, 0);
  for (int32_t ci = e.begin; ci < e.begin + e.count; ++ci) {
    const InvIndex::Cont& ct = inv.conts[ci];
    if (ct.key < 0 || ct.key >= nblk) continue;
    const uint64_t a = payload(ct);
    dir[ct.key] = ct.type == CONT_BITMAP ? a : (ct.n > 0 ? (a | 1ull | ((uint64_t)ct.n << 48)) : 0);
  }
  C.inv_refs.push_back(col.inv);
  C.set_fix.emplace_back(field, (int64_t)C.set_words.size());
  for (uint64_t d : dir) {
    C.set_words.push_back((uint32_t)d);
    C.set_words.push_back((uint32_t)(d >> 32));
  }
  kl.kind = LEAF_BITDIR;
  return true;
}

// LEAF_BITMAP of several dictIds (or one that emit_bitdir declined): a docId bitmap region of whole 65536-doc
// containers, materialised per query from the container tasks.
void emit_bitmap_tasks(Chunk& C, const Segment* s, const Column& col, const LeafHost& lh, int64_t field) {
  const InvIndex& inv = *col.inv;
  C.inv_refs.push_back(col.inv);
  C.bit_fix.emplace_back(field, C.docbit_words);
  const int64_t nblk = ((int64_t)s->num_docs + 65535) >> 16;
  const size_t t0 = C.bit_tasks.size();
  for (int32_t id : lh.inv_ids) {
    const InvIndex::Entry& e = inv.ids[id];
    for (int32_t ci = e.begin; ci < e.begin + e.count; ++ci) {
      const InvIndex::Cont& ct = inv.conts[ci];
      KBitTask task;
      task.payload = reinterpret_cast<const uint32_t*>(inv.d_block) + ct.word;
      task.type = ct.type;
      task.n = ct.n;
      task.dst = C.docbit_words + (int64_t)ct.key * kContainerWords;
      C.bit_tasks.push_back(task);
    }
  }
  if (lh.inv_ids.size() > 1)  // one dictId's containers are already in key order
    std::stable_sort(C.bit_tasks.begin() + t0, C.bit_tasks.end(),
                     [](const KBitTask& x, const KBitTask& y) { return x.dst < y.dst; });
  size_t ti = t0;
  for (int64_t kb = 0; kb < nblk; ++kb) {
    KBitBlock blk;
    blk.dst = C.docbit_words + kb * kContainerWords;
    blk.task_begin = (int32_t)ti;
    while (ti < C.bit_tasks.size() && C.bit_tasks[ti].dst == blk.dst) ++ti;
    blk.num_tasks = (int32_t)(ti - blk.task_begin);
    C.bit_blocks.push_back(blk);
  }
  C.docbit_words += nblk * kContainerWords;
}

// The record's KLeaf of every leaf of segment s, in evaluation order, and what each kind keeps in the chunk.
// kl_off: the byte offset of kl[0] in the chunk's records.
void emit_leaves(const PlanCtx& cx, const Segment* s, const std::vector<LeafHost>& leaves, KLeaf* kl, int64_t kl_off,
                 Chunk& C) {
  std::array<SketchLeaf, kMaxLeaves> sk;
  choose_sketch_leaves(cx, s, leaves, sk, C);
  for (int k = 0; k < cx.P->num_leaves; ++k) {
    const LeafHost& lh = leaves[cx.perm[k]];
    const Column& col = pred_column(cx.P, s, cx.q, cx.perm[k]);
    const int64_t field = kl_off + (int64_t)(k * sizeof(KLeaf) + offsetof(KLeaf, set));
    kl[k].kind = lh.kind;
    kl[k].negate = lh.negate;
    kl[k].lo = lh.lo;
    kl[k].span = lh.span;
    kl[k].set = nullptr;
    const SketchLeaf* sl = cx.perm[k] < kMaxLeaves && sk[cx.perm[k]].use ? &sk[cx.perm[k]] : nullptr;
    if (sl) {  // the leaf over the column's codes: the same docs match (negate carries over)
      kl[k].fwd = reinterpret_cast<const uint32_t*>(col.d_sketch);
      kl[k].bits = kSketchBits;
      if (lh.kind == LEAF_RANGE) {
        kl[k].lo = sl->lo;
        kl[k].span = sl->span;
      }
    }
    if (lh.kind == LEAF_SET) {
      if (sl) emit_set_words(C, sl->codes, kSketchSetWords, field);
      else emit_set_words(C, lh.set.data(), lh.set.size(), field);
    }
    if (lh.kind == LEAF_RAW_RANGE || lh.kind == LEAF_RAW_IN) emit_raw_task(C, s, col, lh, kl[k], field);
    if (lh.kind == LEAF_EXPR_RANGE || lh.kind == LEAF_EXPR_IN)
      emit_expr_task(C, s, cx.P->leaf_exprs[cx.perm[k]], lh, kl[k], field);
    const bool bitdir = lh.kind == LEAF_BITMAP && lh.inv_ids.size() == 1 && emit_bitdir(C, s, col, lh, kl[k], field);
    if (kl[k].kind >= 0 && kl[k].kind < kLeafKinds) C.leaf_kinds[kl[k].kind]++;
    if (lh.kind == LEAF_BITMAP && !bitdir) emit_bitmap_tasks(C, s, col, lh, field);
  }
}

// Per-segment translation (PredicateEvaluatorProvider + FilterPlanNode per segment) of segments [b, e) into C.  Runs
// on host pool threads for large segment lists: it reads the context and the plan (P is const here and in every
// helper) and writes only its Chunk.  The one writer of the plan is a star-tree segment's plan_star_segment, handed
// cx.P itself, and reached on the sequential path alone (any_star).  g_err is thread-local; the caller copies it into
// Chunk::err.
int plan_range(const PlanCtx& cx, size_t b, size_t e, Chunk& C) {
  const pgpu_plan_s* P = cx.P;
  const int nqc = (int)P->query_cols.size();
  std::vector<LeafHost> leaves(P->num_leaves);
  std::vector<Tri> tri(P->num_leaves);
  std::vector<int> ids_scratch;
  std::vector<uint8_t> rec(P->seg_stride);
  std::unordered_map<uint64_t, SegStats> stat_cache;
  for (size_t i = b; i < e; ++i) {
    Segment* s = P->segs[i];
    Tri whole;
    TRY(translate_leaves(cx, i, leaves, tri, ids_scratch, &whole));
    C.scanned.push_back(0);
    if (whole == T_NONE || s->num_docs == 0) continue;  // EmptyFilterOperator: the segment is not scanned
    C.scanned.back() = 1;
    C.matched++;
    if (cx.exempt_kind && whole == T_ALL && !raw_minmax(cx, s)) C.exempt += s->num_docs;
    if (cx.star_allowed && s->star) {  // only on the sequential path (any_star)
      bool used = false;
      TRY(plan_star_segment(cx.P, i, s, cx.q, cx.star_comps, leaves, &used));
      if (used) continue;
    }
    const int32_t rec_stats = segment_stats(cx, s, leaves, tri, stat_cache, C);
    if (C.sel_docs == 0) estimate_chunk_selectivity(cx, s, leaves, C);
    std::fill(rec.begin(), rec.end(), 0);
    KSegHdr* h = reinterpret_cast<KSegHdr*>(rec.data());
    h->num_docs = s->num_docs;
    h->tile_base = (int32_t)C.tiles;  // chunk-relative
    h->num_tiles = (int32_t)((s->num_docs + kTileDocs - 1) / kTileDocs);
    h->stats = rec_stats;
    C.gathers |= fill_kcols(cx, i, reinterpret_cast<KCol*>(rec.data() + sizeof(KSegHdr)));
    const size_t kl_at = sizeof(KSegHdr) + sizeof(KCol) * nqc;
    emit_leaves(cx, s, leaves, reinterpret_cast<KLeaf*>(rec.data() + kl_at), (int64_t)(C.rec.size() + kl_at), C);
    C.rec.insert(C.rec.end(), rec.begin(), rec.end());
    C.tiles += h->num_tiles;
  }
  return 0;
}

// ------------------------------------------------------------------------------------ launch configuration
// K6's launch shape for the plan's star-tree segments.
void configure_star(PlanCtx& cx) {
  pgpu_plan_s* P = cx.P;
  P->star_segments = (int64_t)P->star.size();
  if (P->star.empty()) return;
  if (P->star_cache_ints < 0) P->star_cache_ints = 0;  // some segment's LUTs do not fit: global reads
  int64_t max_nodes = 0;
  for (const KStarSeg& k : P->star) max_nodes = std::max<int64_t>(max_nodes, k.num_nodes);
  P->star_range_cache = max_nodes * 16 <= 32 * 1024 ? (int32_t)max_nodes : 0;
  const int64_t nseg_launch = std::min<int64_t>((int64_t)P->star.size(), kStarMaxSegs);
  P->star_batches = (int)(((int64_t)P->star.size() + kStarMaxSegs - 1) / kStarMaxSegs);
  const int64_t rc = P->star_range_cache;
  const size_t table_bytes = P->mode == MODE_LDS ? (size_t)((cx.nslots * cx.G + 1) & ~int64_t(1)) * 8 : 0;
  P->star_lds_bytes = table_bytes + (size_t)((nseg_launch + 2) & ~int64_t(1)) * 8 + (size_t)((rc + 2) & ~int64_t(1)) * 8 +
                      (size_t)((2 * rc + 3) & ~int64_t(3)) * 4 + (size_t)P->star_cache_ints * 4;
  // K6: persistent workgroups (1024 threads in MODE_LDS, 256 otherwise), one resident wave of them over the
  // CUs; each flushes its table slab once
  const int64_t per_cu = P->mode == MODE_LDS ? std::max<int64_t>(1, std::min<int64_t>(2, (160 * 1024) /
                                                  std::max<size_t>(P->star_lds_bytes, 1))) : 8;
  const int64_t want = P->cfg.star_tree_workgroups;  // pgpu_config
  P->star_chunks = (int)(want > 0 ? want : (int64_t)cx.t->num_cus * per_cu);
}

// The scan kernel's instance and grid.
void configure_scan_grid(PlanCtx& cx, int64_t tile_base) {
  pgpu_table_s* t = cx.t;
  pgpu_plan_s* P = cx.P;
  // Dense instance when tiles are expected to hold >= 8 matches per 32-doc group on average: below that the sparse
  // instance's per-match batches win (measured on MI355X, r04 session x: the C4 scan path at 15 % selectivity
  // 195 -> 170 us with the sparse instance; C2 at 50 % 577 us dense vs 1468 sparse).  pgpu_config.dense_selectivity.
  P->dense = P->mode != MODE_HASH && P->sel_estimate >= P->cfg.dense_selectivity;
  bool f64 = false;
  for (int k : P->slot_kind) f64 |= k == SLOT_SUM_F64;
  // dense plans whose group-by columns need no LUT and whose operands no dictionary lookup in any segment, with no
  // double sums (a streamed plan configures before its later chunks are planned: never simple)
  const bool dense_simple = P->dense && !P->gathers && !f64 && !P->fx && P->dc.empty() && P->tile_bound == 0;
  // the sparse instance with the index + scan pair: two-leaf AND plans with an in-place index leaf
  const bool pair = !P->dense && P->pure_and && P->num_leaves == 2 && P->leaf_kinds[LEAF_BITDIR] > 0;
  const bool fast = !P->dense && !pair && P->pure_and && P->num_leaves <= kFastLeaves;
  P->fast_wide = fast && P->sel_estimate >= 1.0 / 16;
  // plans with DISTINCTCOUNT and plans with SLOT_SUM_FX slots launch their own instances whatever the filter
  P->variant = !P->exprs.empty() ? (P->dense ? kScanExprDense : kScanExprSparse)
               : !P->pct.empty() ? (P->dense ? kScanHistDense : kScanHistSparse)
               : !P->dc.empty() ? (P->dense ? kScanDcDense : kScanDcSparse)
               : P->fx        ? (P->dense ? kScanFxDense : kScanFxSparse)
               : dense_simple ? kScanDenseSimple
               : P->dense     ? kScanDense
               : pair         ? kScanPair
               : P->fast_wide ? kScanFastWide
               : fast         ? kScanFast
                              : kScanSparse;
  int per_cu;  // resident workgroups per CU
  {
    static std::mutex occ_mu;
    static std::map<std::tuple<int, int, int, size_t>, int> occ_cache;  // (device, mode, variant, lds) -> per CU
    std::lock_guard<std::mutex> g(occ_mu);
    const auto k = std::make_tuple(t->device, (int)P->mode, (int)P->variant, P->lds_bytes);
    auto it = occ_cache.find(k);
    if (it == occ_cache.end()) it = occ_cache.emplace(k, occupancy_scan(P->mode, P->variant, P->lds_bytes)).first;
    per_cu = it->second;
  }
  if (per_cu <= 0) per_cu = 1;
  per_cu = std::min(per_cu, 4);
  P->grid = (int)std::max<int64_t>(1, std::min<int64_t>(tile_base, (int64_t)t->num_cus * per_cu));
  // a multiple of the 8 XCDs (the kernel's XCD-aware tile order): rounded up when every tile has a workgroup of its
  // own and the resident capacity allows -- rounded down, an XCD's eighth of the tiles would outnumber its
  // workgroups and one of them would scan two tiles in a row (C1: 492 tiles on 488 workgroups)
  if (P->grid >= 64)
    P->grid = (P->grid == tile_base && ((P->grid + 7) & ~7) <= (int64_t)t->num_cus * per_cu) ? (P->grid + 7) & ~7
                                                                                                : P->grid & ~7;
}

// STATS_LEAP2 bytes of a workgroup's tiles are buffered in LDS (one per tile and wave) until the end of the scan: at
// most kLeapLdsTiles tiles per workgroup (more workgroups than resident ones for huge plans).  Room for the longest
// run of any launch of the plan, weighted by CU slot or not (scan_leap_tiles, tile_split.h); the weights of a launch
// whose runs would not fit are declined (set_slot_weights).  The grid's occupancy was queried without these bytes,
// as it always was.
void reserve_leap2(PlanCtx& cx, int64_t tile_base) {
  pgpu_plan_s* P = cx.P;
  if (!P->any_leap2 && !(cx.se && P->in_kernel_stats)) return;
  P->leap_reserved = true;
  const int64_t need = (tile_base + kLeapLdsTiles - 4) / (kLeapLdsTiles - 3);
  if (P->grid < need) P->grid = (int)((need + 7) & ~int64_t(7));
  P->leap_tiles = scan_leap_tiles(tile_base, P->grid, cx.t->num_cus, P->cfg.slot_weight_step);
  P->lds_bytes += (size_t)scan_lds_maps_bytes(P->leap_tiles);
}

// The record streams of a partitioned plan: one per (query column, integer or double) its slots read.  (The W digit
// slots of a column: one stream of its doubles, split where the records are accumulated.)
void partition_streams(const pgpu_plan_s* P, std::vector<int32_t>* scol, std::vector<int32_t>* sf64,
                       std::vector<int32_t>* sstream) {
  const int nslots = (int)P->slot_kind.size();
  sstream->assign(nslots, -1);
  for (int sl = 1; sl < nslots; ++sl) {
    const int f64 = P->slot_kind[sl] == SLOT_SUM_F64 || P->slot_fx[sl] >= 0 ? 1 : 0;
    int k = -1;
    for (size_t j = 0; j < scol->size(); ++j)
      if ((*scol)[j] == P->slot_col[sl] && (*sf64)[j] == f64) k = (int)j;
    if (k < 0) { scol->push_back(P->slot_col[sl]); sf64->push_back(f64); k = (int)scol->size() - 1; }
    (*sstream)[sl] = k;
  }
}

// Record value widths of a partitioned plan: u32 values when every stream is an integer column whose values fit
// int32 in every segment; with one such stream, its value range, for packing values into the coarse records
// (KPartParams.pack_bits).
void partition_value_widths(pgpu_plan_s* P) {
  bool v32 = true;
  for (size_t j = 0; j < P->stream_col.size() && v32; ++j) {
    const int c = P->query_cols[P->stream_col[j]];
    if (P->stream_f64[j]) v32 = false;
    else if (c != kDocIdColumn) {
      const IntRange r = int_column_range(P->segs, c);
      v32 = r.known && (r.lo > r.hi || (r.lo >= INT32_MIN && r.hi <= INT32_MAX));
    }
  }
  P->part_val32 = v32;
  P->part_pack_range = -1;
  if (v32 && P->stream_col.size() == 1 && P->query_cols[P->stream_col[0]] != kDocIdColumn) {
    const IntRange r = int_column_range(P->segs, P->query_cols[P->stream_col[0]]);
    if (r.lo <= r.hi) {
      P->part_pack_min = r.lo;
      P->part_pack_range = r.hi - r.lo;
    }
  }
}

// Large dense tables: partitioned group-by (partition.h) instead of random global atomics; sparse hash key spaces
// below 2^31: the same passes over hashed partitions (K8h) instead of the global hash table.
void configure_partitions(PlanCtx& cx, int64_t tile_base) {
  pgpu_plan_s* P = cx.P;
  const int nslots = cx.nslots;
  if (!part_eligible(P, nslots, cx.G) || !P->star.empty() || tile_base <= 0 || P->total_docs >= (int64_t)UINT32_MAX)
    return;
  const bool hash_part = part_hash_eligible(P, cx.G);
  int shift = 16;
  while (shift > 8 && ((int64_t)nslots << shift) * 8 > kPartLds) --shift;
  int64_t parts = (cx.G + (int64_t(1) << shift) - 1) >> shift;
  int pbits = 0, sbits = 0;
  if (hash_part) {
    hash_part_bits(P->cfg, P->group_bound, nslots, &pbits, &sbits);
    shift = 0;
    parts = int64_t(1) << pbits;
  }
  std::vector<int32_t> scol, sf64, sstream;
  partition_streams(P, &scol, &sf64, &sstream);
  const int64_t rec_bytes = P->total_docs * ((hash_part ? 4 : 2) + 8 * (int64_t)scol.size());
  if (parts > kMaxParts || rec_bytes > kPartMaxRecordBytes || (hash_part && (int)scol.size() > kHashPartStreams) ||
      !part_pass_shape(P, parts, tile_base))
    return;
  P->partitioned = true;
  P->part_hash = hash_part;
  if (hash_part) P->pack_slot = -1;  // K8h accumulates every slot itself (no packed global words)
  P->part_pbits = pbits;
  P->part_sbits = sbits;
  P->part_shift = shift;
  P->num_parts = (int)parts;
  P->stream_col = scol;
  P->stream_f64 = sf64;
  P->slot_stream = sstream;
  partition_value_widths(P);
}

// Launch configuration once the tiles are known (tile_base: their number, or an upper bound for streamed plans).
int configure(PlanCtx& cx, int64_t tile_base) {
  cx.P->num_tiles = tile_base;
  if (tile_base > INT32_MAX) return fail(PGPU_ERR_UNSUPPORTED, "too many tiles in one plan");
  configure_star(cx);
  configure_scan_grid(cx, tile_base);
  reserve_leap2(cx, tile_base);
  configure_partitions(cx, tile_base);
  return 0;
}

// Appends a planned chunk to the plan; tile_shift is added to its records' chunk-relative tile_base (0 keeps
// them relative, as a streamed launch of the chunk reads them).
void merge_chunk(pgpu_plan_s* P, Chunk& C, int64_t tile_shift) {
  if (P->set_words.size() & 1) P->set_words.push_back(0);  // chunk words keep their 8-byte alignment
  const int64_t rec0 = (int64_t)P->segrec.size(), set0 = (int64_t)P->set_words.size();
  if (tile_shift)
    for (size_t r = 0; r < C.rec.size(); r += P->seg_stride)
      reinterpret_cast<KSegHdr*>(C.rec.data() + r)->tile_base += (int32_t)tile_shift;
  for (auto& f : C.set_fix) P->set_fix.emplace_back(rec0 + f.first, set0 + f.second);
  for (auto& f : C.bit_fix) P->bit_fix.emplace_back(rec0 + f.first, P->docbit_words + f.second);
  for (KBitBlock blk : C.bit_blocks) {
    blk.dst += P->docbit_words;
    blk.task_begin += (int32_t)P->bit_tasks.size();
    P->bit_blocks.push_back(blk);
  }
  P->bit_tasks.insert(P->bit_tasks.end(), C.bit_tasks.begin(), C.bit_tasks.end());
  for (KRawTask rt : C.raw_tasks) {
    rt.dst += P->docbit_words;
    if (rt.kind == LEAF_RAW_IN) rt.lo += (int64_t)P->raw_vals.size();
    P->raw_tasks.push_back(rt);
  }
  P->raw_vals.insert(P->raw_vals.end(), C.raw_vals.begin(), C.raw_vals.end());
  for (KExprLeafTask et : C.expr_tasks) {
    et.dst += P->docbit_words;
    if (et.kind == LEAF_RAW_IN) et.lo += (int64_t)P->expr_vals.size();
    P->expr_tasks.push_back(et);
  }
  P->expr_vals.insert(P->expr_vals.end(), C.expr_vals.begin(), C.expr_vals.end());
  P->inv_refs.insert(P->inv_refs.end(), C.inv_refs.begin(), C.inv_refs.end());
  for (auto& g : C.generic) {
    g.rec += rec0 / std::max(P->seg_stride, 1);
    g.out_word = P->generic_words;
    P->generic_words += (int64_t)P->num_leaves * (((int64_t)g.num_docs + 31) / 32);
    P->generic.push_back(std::move(g));
  }
  P->any_leap2 |= C.any_leap2;
  P->gathers |= C.gathers;
  P->docbit_words += C.docbit_words;
  P->segrec.insert(P->segrec.end(), C.rec.begin(), C.rec.end());
  P->set_words.insert(P->set_words.end(), C.set_words.begin(), C.set_words.end());
  P->seg_scanned.insert(P->seg_scanned.end(), C.scanned.begin(), C.scanned.end());
  P->segments_matched_filter += C.matched;
  P->scanned_entries_model += C.entries;
  P->post_exempt_docs += C.exempt;
  for (int k = 0; k < kLeafKinds; ++k) P->leaf_kinds[k] += C.leaf_kinds[k];
  for (int k = 0; k < 2; ++k) P->sketch_leaves[k] += C.sketch_leaves[k];
  if (P->sel_docs == 0 && C.sel_docs) { P->sel_estimate = C.sel; P->sel_docs = C.sel_docs; }
}

// ------------------------------------------------------------------------------------ drivers
// Streamed plan (pgpu_plan_create_execute): equal chunks of segments, each launched as soon as it is planned,
// so the GPU scans chunk c while the host translates chunk c + 1 (Pinot plans and runs each segment's
// operator on its own worker thread, BaseCombineOperator.java:85-115).
int run_streamed(PlanCtx& cx, int stream_chunks) {
  const pgpu_query* q = cx.q;
  pgpu_plan_s* P = cx.P;
  const StreamExec* se = cx.se;
  const size_t nseg = P->segs.size();
  for (Segment* s : P->segs) {
    P->tile_bound += (s->num_docs + kTileDocs - 1) / kTileDocs;
    for (int l = 0; l < P->num_leaves; ++l) {
      const int ty = q->predicates[l].type;
      if (ty == PGPU_PRED_IN || ty == PGPU_PRED_NOT_IN || ty == PGPU_PRED_REGEXP_LIKE)
        P->set_words_bound += ((int64_t)pred_column(P, s, q, l).card + 31) / 32;
    }
  }
  if (!P->scratch) return fail(PGPU_ERR_INVALID_ARGUMENT, "streamed plan without scratch");
  ExecCtx X;
  int64_t tile_off = 0;
  cx.mark();
  for (int c = 0; c < stream_chunks; ++c) {
    Chunk C;
    C.rec.reserve((nseg / stream_chunks + 1) * (size_t)P->seg_stride);
    TRY(plan_range(cx, nseg * c / stream_chunks, nseg * (c + 1) / stream_chunks, C));
    LaunchChunk L;
    L.rec_begin = (int64_t)(P->segrec.size() / P->seg_stride);
    L.fix_begin = (int64_t)P->set_fix.size();
    L.set_begin = (int64_t)P->set_words.size();
    L.tile_begin = tile_off;
    merge_chunk(P, C, 0);
    L.num_recs = (int64_t)(P->segrec.size() / P->seg_stride) - L.rec_begin;
    L.fix_end = (int64_t)P->set_fix.size();
    L.set_end = (int64_t)P->set_words.size();
    L.num_tiles = C.tiles;
    tile_off += C.tiles;
    P->chunks.push_back(L);
    if (c == 0) {
      TRY(configure(cx, P->tile_bound));
      TRY(exec_prologue(P, se->stream, se->d_table, stream_chunks, X));
    }
    TRY(exec_upload_chunk(P, se->stream, X, L));
    TRY(exec_launch_chunk(P, se->stream, X, L, c));
  }
  cx.mark();
  P->num_tiles = tile_off;
  TRY(exec_epilogue(P, se->stream, X));
  if (trace_on())
    fprintf(stderr, "[pgpu] plan_create (streamed, %d launches): %.1f us (%zu segments)\n", stream_chunks,
            now_us() - cx.t_start, P->segs.size());
  return 0;
}

// Small plans (C1: one 1M-doc segment = 123 tiles on 256 CUs): split every tile into 2 or 4 so that at least two
// tiles per CU run.  The scan kernel's direct path only: not with leap-frog statistics (their per-(tile, wave)
// bytes are whole 32-doc groups) nor the partitioned group-by (its own passes).  Returns the tiles after the split.
int64_t split_small_tiles(PlanCtx& cx, int64_t tile_base) {
  pgpu_plan_s* P = cx.P;
  // (only the dense half of part_eligible: such a table is not split even with partitioned_group_by off; hashed
  // partitions are)
  if (tile_base <= 0 || tile_base >= 2 * (int64_t)cx.t->num_cus || P->any_leap2 || !P->star.empty() ||
      dense_part_eligible(P, cx.nslots, cx.G))
    return tile_base;
  int sh = 1;
  while (sh < 2 && (tile_base << sh) < 2 * (int64_t)cx.t->num_cus) ++sh;
  P->tile_shift = sh;
  for (size_t r = 0; r + sizeof(KSegHdr) <= P->segrec.size(); r += P->seg_stride) {
    KSegHdr* h = reinterpret_cast<KSegHdr*>(P->segrec.data() + r);
    h->tile_base <<= sh;
    h->num_tiles <<= sh;
  }
  return tile_base << sh;
}

// One launch: the segments translated in contiguous chunks, on the host worker pool for large segment lists, then
// concatenated in segment order and configured.
int run_pooled(PlanCtx& cx) {
  pgpu_plan_s* P = cx.P;
  const size_t nseg = P->segs.size();
  const int nchunks = cx.any_star ? 1 : (int)std::min<size_t>(host_pool().size() + 1, (nseg + plan_chunk_segs(P->cfg) - 1) / plan_chunk_segs(P->cfg));
  std::vector<Chunk> chunks(std::max(nchunks, 1));
  auto run_chunk = [&](int c) {
    Chunk& C = chunks[c];
    C.rec.reserve((nseg / chunks.size() + 1) * (size_t)P->seg_stride);
    C.rc = plan_range(cx, nseg * c / chunks.size(), nseg * (c + 1) / chunks.size(), C);
    if (C.rc) C.err = g_err;
  };
  cx.mark();
  if (chunks.size() == 1) run_chunk(0);
  else host_pool().run((int)chunks.size(), run_chunk);
  cx.mark();
  int64_t tile_base = 0;
  for (Chunk& C : chunks) {
    if (C.rc) return fail(C.rc, "%s", C.err.c_str());
    merge_chunk(P, C, tile_base);
    tile_base += C.tiles;
  }
  TRY(configure(cx, split_small_tiles(cx, tile_base)));
  P->chunks.assign(1, LaunchChunk{0, (int64_t)(P->segrec.size() / std::max(P->seg_stride, 1)), 0, P->num_tiles, 0,
                                  (int64_t)P->set_fix.size(), 0, (int64_t)P->set_words.size()});
  if (trace_on())
    fprintf(stderr, "[pgpu] plan_create: %.1f us (%zu segments; setup %.1f, ensure %.1f, translate %.1f, rest %.1f)\n",
            now_us() - cx.t_start, P->segs.size(), cx.tr[0] - cx.t_start, cx.tr[1] - cx.tr[0], cx.tr[2] - cx.tr[1],
            now_us() - cx.tr[2]);
  return 0;
}

}  // namespace

// The phases in order: each reads what the earlier ones left in the plan and the context.
int plan_create_impl(pgpu_table_s* t, const int64_t* handles, int32_t nsegs, const pgpu_query* q, pgpu_plan_s* P,
                     const StreamExec* se) {
  if (!q) return fail(PGPU_ERR_INVALID_ARGUMENT, "null query");
  PlanCtx cx{t, q, P, se};
  cx.t_start = trace_on() ? now_us() : 0;
  P->cfg = table_config(t);
  {
    std::lock_guard<std::mutex> g(t->cfg_mu);
    P->sketch_on = t->sketch_min_bits > 0;
  }
  // num_group_by == 0: aggregation-only (AggregationOperator, core/operator/query/AggregationOperator.java:58-95):
  // one accumulator row (key space G = 1), reduced per wave before any atomic.
  if (q->num_group_by < 0) return fail(PGPU_ERR_INVALID_ARGUMENT, "negative group-by count");
  if (q->num_group_by > kMaxKeys) return fail(PGPU_ERR_UNSUPPORTED, "more than %d group-by columns", kMaxKeys);
  if (q->num_predicates > kMaxLeaves) return fail(PGPU_ERR_UNSUPPORTED, "more than %d predicates", kMaxLeaves);
  if (q->num_filter_ops > kMaxOps) return fail(PGPU_ERR_UNSUPPORTED, "filter program longer than %d", kMaxOps);
  P->table = t;
  P->end_time_ms = q->end_time_ms;
  TRY(acquire_segments(cx, handles, nsegs));
  TRY(bind_query_columns(cx));
  TRY(compile_filter(q, &P->ops, &P->pure_and, &P->max_depth));
  TRY(assign_slots(cx));
  note_groups_limit(cx);
  TRY(build_device_arrays(cx));
  TRY(run_regex_leaves(cx));
  std::vector<int64_t> kspan;  // per key column: the global ids the filter admits
  TRY(restrict_key_space(cx, &kspan));
  TRY(layout_keys(cx, kspan));
  choose_table_mode(cx);
  TRY(check_distinct_shape(cx));
  TRY(prepare_translation(cx));
  order_leaves(cx);
  const bool partitions = part_eligible(P, cx.nslots, cx.G);
  // CHAIN / LEAP2 statistics need the direct kernel's register fast path (a pure AND of <= kFastLeaves leaves)
  P->in_kernel_stats = P->pure_and && P->num_leaves <= kFastLeaves && !partitions;
  const int stream_chunks = se ? stream_chunk_count(P->cfg, P->segs.size()) : 1;
  if (se && !cx.any_star && !cx.any_inv && !cx.any_raw_leaf && !partitions && stream_chunks > 1)
    return run_streamed(cx, stream_chunks);
  return run_pooled(cx);
}

}  // namespace pgpu
