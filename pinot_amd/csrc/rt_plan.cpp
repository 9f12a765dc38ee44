// rt_plan.cpp -- what query planning is made of: predicate translation, filter folding, star-tree plans, slot and
// partition sizing (rt.h).  plan_create_impl, which puts them together, is rt_plan_create.cpp's.
#include "rt_decls.h"

namespace pgpu {

// Open-addressing table slots for at most `groups` groups: load <= 1/2, a power of two, >= 1024.
int64_t hash_capacity(int64_t groups) {
  const int64_t want = std::max<int64_t>(2 * std::max<int64_t>(groups, 1), 1024);
  int64_t cap = 1;
  while (cap < want) cap <<= 1;
  return cap;
}

// The free scratch that has grown the most: a query then finds its buffers at size, where handing out the first free
// one had a steady stream of repeated queries take a scratch that a smaller query had sized and grow it -- hipFree
// waits for the whole device (C4's star path at 3 queries in flight: one launch of 7 ms in a 20-query run).
Scratch* acquire_scratch(pgpu_table_s* t) {
  std::lock_guard<std::mutex> g(t->mu);
  std::unique_ptr<Scratch>* best = nullptr;
  size_t best_bytes = 0;
  for (auto& s : t->scratch_pool)
    if (s && (!s->abandoned || hipEventQuery(s->busy) != hipErrorNotReady)) {
      const size_t b = s->footprint();
      if (!best || b > best_bytes) {
        best = &s;
        best_bytes = b;
      }
    }
  if (!best) return new Scratch();
  Scratch* r = best->release();
  best->reset();
  r->abandoned = false;
  return r;
}
void release_scratch(pgpu_table_s* t, Scratch* s) {
  if (!s) return;
  std::lock_guard<std::mutex> g(t->mu);
  for (auto& p : t->scratch_pool)
    if (!p) { p.reset(s); return; }
  t->scratch_pool.emplace_back(s);
}


// Literal conversion per column type; false = BadQueryRequestException (PredicateEvaluatorProvider.java:85-88).
bool parse_literal(int type, const char* lit, bool allow_star, Literal* out) {
  if (allow_star && strcmp(lit, "*") == 0) { out->star = true; return true; }
  switch (type) {
    case PGPU_INT: return parse_long(lit, INT32_MIN, INT32_MAX, &out->i);
    case PGPU_LONG: return parse_long(lit, INT64_MIN, INT64_MAX, &out->i);
    case PGPU_FLOAT:
      if (!parse_double(lit, &out->d)) return false;
      out->d = (double)(float)out->d;
      return true;
    case PGPU_DOUBLE: return parse_double(lit, &out->d);
    default: out->s = lit; return true;
  }
}


int insertion_index(const Column& c, const Literal& v) {
  const Dict& d = c.dict;
  int lo = 0, hi = (int)d.size() - 1;
  switch (d.type) {
    case PGPU_INT: case PGPU_LONG:
      return sorted_search<int64_t>(d.iv, v.i);
    case PGPU_FLOAT: case PGPU_DOUBLE:
      return sorted_search<double>(d.dv, v.d);
    default: {
      const uint8_t* lv = reinterpret_cast<const uint8_t*>(v.s.data());
      const size_t ln = v.s.size();
      if (c.padding == 0) {
        while (lo <= hi) {
          const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
          const std::string& m = d.sv[mid];
          const int r = cmp_bytes(reinterpret_cast<const uint8_t*>(m.data()), m.size(), lv, ln);
          if (r < 0) lo = mid + 1;
          else if (r > 0) hi = mid - 1;
          else return mid;
        }
      } else {  // legacy non-zero padding: padded comparison (BaseImmutableDictionary.java:215-228)
        std::string padded(v.s);
        if ((int)padded.size() < c.entry_width) padded.append(c.entry_width - padded.size(), (char)c.padding);
        while (lo <= hi) {
          const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
          const uint8_t* m = c.raw_dict.data() + (int64_t)mid * c.entry_width;
          const int r = cmp_bytes(m, c.entry_width, reinterpret_cast<const uint8_t*>(padded.data()), padded.size());
          if (r < 0) lo = mid + 1;
          else if (r > 0) hi = mid - 1;
          else return mid;
        }
      }
      return -(lo + 1);
    }
  }
}

// Converts the literals of predicate `p` for a column of `type`.
int parse_predicate(int type, const pgpu_predicate& p, ParsedPred* out) {
  const int need = p.type == PGPU_PRED_RANGE ? 2 : 1;
  if (p.num_values < need) return fail(PGPU_ERR_INVALID_ARGUMENT, "predicate on column %d needs %d value(s)", p.column, need);
  out->lits.resize(p.num_values);
  for (int i = 0; i < p.num_values; ++i)
    if (!parse_literal(type, p.values[i], p.type == PGPU_PRED_RANGE, &out->lits[i]))
      return fail(PGPU_ERR_BAD_QUERY, "BadQueryRequestException: cannot convert '%s' to the type of column %d",
                  p.values[i], p.column);
  return 0;
}

// FilterOperatorUtils.getLeafFilterOperator (FilterOperatorUtils.java:72-79): an EQ / NOT_EQ / IN / NOT_IN
// predicate on a column with an inverted index (and not sorted: the sorted index wins) becomes a
// BitmapBasedFilterOperator.  The leaf keeps its negate flag: flip(OR(bitmaps of the literals' dictIds)) over
// [0, numDocs) equals the reference's OR over the non-matching dictIds (BitmapBasedFilterOperator.java:73-98).
void to_inverted_leaf(const Column& c, const pgpu_predicate& p, const Segment& s, LeafHost* L) {
  if (!c.inv || c.sorted || (L->kind != LEAF_RANGE && L->kind != LEAF_SET)) return;
  if (p.type != PGPU_PRED_EQ && p.type != PGPU_PRED_NOT_EQ && p.type != PGPU_PRED_IN && p.type != PGPU_PRED_NOT_IN)
    return;
  L->inv_ids.clear();
  if (L->kind == LEAF_RANGE) {
    for (uint32_t i = 0; i < L->span; ++i) L->inv_ids.push_back((int32_t)(L->lo + i));
  } else {
    for (size_t w = 0; w < L->set.size(); ++w)
      for (uint32_t bits = L->set[w]; bits; bits &= bits - 1)
        L->inv_ids.push_back((int32_t)(w * 32 + __builtin_ctz(bits)));
  }
  int64_t docs = 0;
  for (int32_t id : L->inv_ids) docs += c.inv->ids[id].docs;
  L->inv_frac = (double)docs / std::max(1, s.num_docs);
  L->kind = LEAF_BITMAP;
}

// Translates predicate `p` against one segment's column dictionary (dictionary-based PredicateEvaluators).
// `ids` is caller-owned scratch.
int translate_predicate_dict(const Column& c, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L,
                             std::vector<int>& ids);

// Dictionary-space translation, then on a sorted column a dictId range becomes the docId range of the
// SortedIndexBasedFilterOperator (SortedIndexBasedFilterOperator.java:51-125; dictIds [lo, hi) own docs
// [start(lo), start(hi)) of the SortedIndexReaderImpl pairs).
int translate_predicate(const Column& c, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L,
                        std::vector<int>& ids) {
  TRY(translate_predicate_dict(c, p, pp, L, ids));
  if (c.sorted && L->kind == LEAF_RANGE) {
    const int32_t d0 = c.sorted_start[L->lo], d1 = c.sorted_start[L->lo + L->span];
    L->dict_lo = L->lo;
    L->dict_span = L->span;
    L->kind = LEAF_DOCRANGE;
    L->lo = (uint32_t)d0;
    L->span = (uint32_t)std::max(0, d1 - d0);
  }
  return 0;
}

int translate_predicate_dict(const Column& c, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L,
                             std::vector<int>& ids) {
  const int32_t card = c.card;
  switch (p.type) {
    case PGPU_PRED_EQ: {  // EqualsPredicateEvaluatorFactory.java:86-99
      const int ins = insertion_index(c, pp.lits[0]);
      if (ins < 0) L->kind = LEAF_NONE;
      else if (card == 1) L->kind = LEAF_ALL;
      else { L->kind = LEAF_RANGE; L->lo = ins; L->span = 1; }
      return 0;
    }
    case PGPU_PRED_NOT_EQ: {  // NotEqualsPredicateEvaluatorFactory.java:88-102
      const int ins = insertion_index(c, pp.lits[0]);
      if (ins < 0) L->kind = LEAF_ALL;
      else if (card == 1) L->kind = LEAF_NONE;
      else { L->kind = LEAF_RANGE; L->lo = ins; L->span = 1; L->negate = 1; }
      return 0;
    }
    case PGPU_PRED_IN: case PGPU_PRED_NOT_IN: {  // InPredicateEvaluatorFactory.java:138-154, NotIn...:140-160
      ids.clear();
      for (const Literal& v : pp.lits) {
        const int ins = insertion_index(c, v);
        if (ins >= 0) ids.push_back(ins);
      }
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
      const int n = (int)ids.size();
      const bool in = p.type == PGPU_PRED_IN;
      if (n == 0) { L->kind = in ? LEAF_NONE : LEAF_ALL; return 0; }
      if (n == card) { L->kind = in ? LEAF_ALL : LEAF_NONE; return 0; }
      L->negate = in ? 0 : 1;
      if (ids.back() - ids.front() + 1 == n) {  // contiguous dictIds: a range test
        L->kind = LEAF_RANGE;
        L->lo = ids.front();
        L->span = n;
      } else {
        L->kind = LEAF_SET;
        L->set.assign(((size_t)card + 31) / 32, 0u);
        for (int id : ids) L->set[id >> 5] |= 1u << (id & 31);
      }
      return 0;
    }
    case PGPU_PRED_RANGE: {  // SortedDictionaryBasedRangePredicateEvaluator (RangePredicateEvaluatorFactory.java:115-159)
      int start, end;
      if (pp.lits[0].star) start = 0;
      else {
        const int ins = insertion_index(c, pp.lits[0]);
        start = ins < 0 ? -(ins + 1) : (p.lower_inclusive ? ins : ins + 1);
      }
      if (pp.lits[1].star) end = card;
      else {
        const int ins = insertion_index(c, pp.lits[1]);
        end = ins < 0 ? -(ins + 1) : (p.upper_inclusive ? ins + 1 : ins);
      }
      const int nm = end - start;
      if (nm <= 0) L->kind = LEAF_NONE;
      else if (nm == card) L->kind = LEAF_ALL;
      else { L->kind = LEAF_RANGE; L->lo = start; L->span = nm; }
      return 0;
    }
    default:
      return fail(PGPU_ERR_UNSUPPORTED, "predicate type %d is not on the GPU path", p.type);
  }
}

// Raw-value predicate evaluators (no dictionary; BaseRawValueBasedPredicateEvaluator subclasses, never always-true /
// -false for FilterPlanNode): the leaf tests the column's per-doc int64 keys -- the value for INT / LONG, the
// order-preserving key of the double for FLOAT / DOUBLE (NaN canonical) -- against
//   RANGE (RangePredicateEvaluatorFactory.java:60-102, 268-448): unbounded = inclusive MIN / MAX (+-inf); Java's
//          comparisons turned into inclusive key bounds (exclusive: the next representable value; 0.0 and -0.0
//          compare equal, NaN never matches);
//   EQ / NOT_EQ (EqualsPredicateEvaluatorFactory.java:60-70 `==`, NotEquals `!=`): the range [v, v] (negated);
//   IN / NOT_IN (InPredicateEvaluatorFactory.java:69-126): fastutil Int/Long/Float/DoubleOpenHashSet.contains --
//          bit equality (Float.floatToIntBits / Double.doubleToLongBits: 0.0 != -0.0, NaN == NaN).
void translate_raw_predicate(int type, const pgpu_predicate& p, const ParsedPred& pp, LeafHost* L) {
  L->raw.clear();
  L->negate = 0;
  const bool fp = is_fp_type(type);
  auto empty = [&] { L->kind = LEAF_RAW_RANGE; L->raw = {1, 0}; };
  auto fkey = [](double v) { return double_key(std::isnan(v) ? kCanonicalNaN : v); };
  switch (p.type) {
    case PGPU_PRED_EQ: case PGPU_PRED_NOT_EQ: {
      L->negate = p.type == PGPU_PRED_NOT_EQ;
      L->kind = LEAF_RAW_RANGE;
      if (!fp) { L->raw = {pp.lits[0].i, pp.lits[0].i}; return; }
      const double v = pp.lits[0].d;
      if (std::isnan(v)) { empty(); L->negate = p.type == PGPU_PRED_NOT_EQ; return; }
      if (v == 0.0) L->raw = {fkey(-0.0), fkey(0.0)};
      else L->raw = {fkey(v), fkey(v)};
      return;
    }
    case PGPU_PRED_IN: case PGPU_PRED_NOT_IN: {
      L->negate = p.type == PGPU_PRED_NOT_IN;
      L->kind = LEAF_RAW_IN;
      for (const Literal& v : pp.lits) L->raw.push_back(fp ? fkey(v.d) : v.i);
      std::sort(L->raw.begin(), L->raw.end());
      L->raw.erase(std::unique(L->raw.begin(), L->raw.end()), L->raw.end());
      L->span = (uint32_t)L->raw.size();
      return;
    }
    default: {  // RANGE
      L->kind = LEAF_RAW_RANGE;
      const Literal& a = pp.lits[0];
      const Literal& b = pp.lits[1];
      if (!fp) {
        const int64_t tmin = type == PGPU_INT ? INT32_MIN : INT64_MIN, tmax = type == PGPU_INT ? INT32_MAX : INT64_MAX;
        int64_t lo = a.star ? tmin : a.i, hi = b.star ? tmax : b.i;
        if (!a.star && !p.lower_inclusive) { if (lo == INT64_MAX) { empty(); return; } ++lo; }
        if (!b.star && !p.upper_inclusive) { if (hi == INT64_MIN) { empty(); return; } --hi; }
        L->raw = {lo, hi};
        return;
      }
      const double inf = std::numeric_limits<double>::infinity();
      double lo = a.star ? -inf : a.d, hi = b.star ? inf : b.d;
      if (std::isnan(lo) || std::isnan(hi)) { empty(); return; }
      int64_t klo, khi;
      if (a.star || p.lower_inclusive) klo = lo == 0.0 ? fkey(-0.0) : fkey(lo);
      else if (lo == inf) { empty(); return; }
      else klo = fkey(lo == 0.0 ? std::nextafter(0.0, inf) : std::nextafter(lo, inf));
      if (b.star || p.upper_inclusive) khi = hi == 0.0 ? fkey(0.0) : fkey(hi);
      else if (hi == -inf) { empty(); return; }
      else khi = fkey(hi == 0.0 ? std::nextafter(-0.0, -inf) : std::nextafter(hi, -inf));
      L->raw = {klo, khi};
      return;
    }
  }
}

// Constant folding of the program against the leaves' constants (FilterPlanNode.java:146-176).
// Fraction of docs the filter program passes if every dictId were equally frequent (leaf fractions combined as
// independent events).  Only picks the scan kernel instance (dense / sparse): never affects results.
double estimate_selectivity(const std::vector<int32_t>& ops, const std::vector<double>& leaf) {
  double st[kMaxOps];
  int sp = 0;
  for (int32_t e : ops) {
    const int op = e >> 16, arg = e & 0xFFFF;
    if (op == OP_LEAF) st[sp++] = leaf[arg];
    else if (op == OP_NOT) st[sp - 1] = 1.0 - st[sp - 1];
    else {
      double x = op == OP_AND ? 1.0 : 0.0;
      for (int j = sp - arg; j < sp; ++j) x = op == OP_AND ? x * st[j] : 1.0 - (1.0 - x) * (1.0 - st[j]);
      sp -= arg;
      st[sp++] = x;
    }
  }
  return sp == 0 ? 1.0 : st[sp - 1];
}

Tri fold_program(const std::vector<int32_t>& ops, const std::vector<Tri>& leaf) {
  Tri st[kMaxOps];
  int sp = 0;
  for (int32_t e : ops) {
    const int op = e >> 16, arg = e & 0xFFFF;
    if (op == OP_LEAF) st[sp++] = leaf[arg];
    else if (op == OP_NOT) {
      Tri& x = st[sp - 1];
      x = x == T_ALL ? T_NONE : x == T_NONE ? T_ALL : T_VAR;
    } else {
      bool any_none = false, any_all = false, all_all = true, all_none = true;
      for (int j = sp - arg; j < sp; ++j) {
        any_none |= st[j] == T_NONE;
        any_all |= st[j] == T_ALL;
        all_all &= st[j] == T_ALL;
        all_none &= st[j] == T_NONE;
      }
      sp -= arg;
      if (op == OP_AND) st[sp++] = any_none ? T_NONE : all_all ? T_ALL : T_VAR;
      else st[sp++] = any_all ? T_ALL : all_none ? T_NONE : T_VAR;
    }
  }
  return sp == 0 ? T_ALL : st[sp - 1];
}

// ------------------------------------------------------------------------------------------------ star-tree plans
// The filter as a star-tree sees it: composites (one leaf, or an OR of leaves on one column) that are ANDed
// (StarTreeUtils.extractPredicateEvaluatorsMap / isOrClauseValidForStarTree, core/startree/StarTreeUtils.java:
// 88-218).  False for other shapes (NOT, AND under OR, OR across columns): those segments use the scan path, which
// returns the same result.
bool star_composites(const std::vector<int32_t>& ops, const pgpu_query* q, std::vector<std::vector<int>>* out) {
  struct Node {
    int type;  // 0 leaf, 1 OR on one column, 2 AND
    int col;
    std::vector<int> leaves;
    std::vector<std::vector<int>> comps;
  };
  std::vector<Node> st;
  for (int32_t e : ops) {
    const int op = e >> 16, arg = e & 0xFFFF;
    if (op == OP_LEAF) {
      st.push_back({0, q->predicates[arg].column, {arg}, {}});
    } else if (op == OP_NOT) {
      return false;
    } else if (op == OP_OR) {
      Node n{1, -1, {}, {}};
      for (int j = (int)st.size() - arg; j < (int)st.size(); ++j) {
        if (st[j].type == 2) return false;
        if (n.col >= 0 && st[j].col != n.col) return false;
        n.col = st[j].col;
        n.leaves.insert(n.leaves.end(), st[j].leaves.begin(), st[j].leaves.end());
      }
      st.resize(st.size() - arg);
      st.push_back(std::move(n));
    } else {
      Node n{2, -1, {}, {}};
      for (int j = (int)st.size() - arg; j < (int)st.size(); ++j) {
        if (st[j].type == 2) n.comps.insert(n.comps.end(), st[j].comps.begin(), st[j].comps.end());
        else n.comps.push_back(st[j].leaves);
      }
      st.resize(st.size() - arg);
      st.push_back(std::move(n));
    }
  }
  out->clear();
  if (st.empty()) return true;
  if (st.back().type == 2) *out = st.back().comps;
  else out->push_back(st.back().leaves);
  return true;
}

// Matching dictIds of one translated leaf over [0, card) as a bitset (PredicateEvaluator.getMatchingDictIds).
void leaf_bitset(const LeafHost& L, int32_t card, std::vector<uint32_t>& w) {
  const size_t nw = ((size_t)card + 31) / 32;
  w.assign(nw, 0u);
  for (int32_t i = 0; i < card; ++i) {
    bool m;
    switch (L.kind) {
      case LEAF_ALL: m = true; break;
      case LEAF_NONE: m = false; break;
      case LEAF_RANGE: m = (uint32_t)i >= L.lo && (uint32_t)i < L.lo + L.span; break;
      case LEAF_DOCRANGE: m = (uint32_t)i >= L.dict_lo && (uint32_t)i < L.dict_lo + L.dict_span; break;
      default: m = (L.set[i >> 5] >> (i & 31)) & 1u; break;
    }
    if (L.kind == LEAF_RANGE || L.kind == LEAF_SET || L.kind == LEAF_DOCRANGE) m ^= L.negate != 0;
    if (m) w[i >> 5] |= 1u << (i & 31);
  }
}

// Plans segment `s` on its star-tree when the query fits it (StarTreeUtils.isFitForStarTree, :151-176, and the
// function-column pairs of the aggregations, :67-86).  *used = false leaves the segment to the scan path.
int plan_star_segment(pgpu_plan_s* P, size_t seg_index, Segment* s, const pgpu_query* q,
                      const std::vector<std::vector<int>>& comps, const std::vector<LeafHost>& leaves, bool* used) {
  *used = false;
  const StarTreeDev* st = s->star.get();
  if (!st || st->num_dims > kMaxStarDims || st->num_nodes < 1 || P->first_doc_slot) return 0;
  bool has_avg = false;
  int avg_col = -1;
  for (int i = 0; i < q->num_aggs; ++i) {
    if (st->pair(q->aggs[i].fn, q->aggs[i].column) < 0) return 0;
    if (q->aggs[i].fn == PGPU_AGG_AVG) { has_avg = true; avg_col = q->aggs[i].column; }
  }
  for (int c : P->key_cols)
    if (st->dim_of(c) < 0) return 0;
  for (int l = 0; l < q->num_predicates; ++l)
    if (st->dim_of(q->predicates[l].column) < 0) return 0;
  KStarSeg k;
  memset(&k, 0, sizeof k);
  k.nodes = st->d_nodes;
  k.num_nodes = st->num_nodes;
  k.num_docs = st->num_docs;
  k.num_dims = st->num_dims;
  for (int d = 0; d < st->num_dims; ++d) {
    k.dim_fwd[d] = st->d_dim_fwd[d];
    k.dim_bits[d] = st->dim_bits[d];
  }
  // slot sources
  const int cnt_pair = st->pair(PGPU_AGG_COUNT, -1);
  const int cnt_m = cnt_pair >= 0 ? cnt_pair : has_avg ? st->pair(PGPU_AGG_AVG, avg_col) : -1;
  if (cnt_m >= 0) {
    k.src_c[0] = st->d_mc[cnt_m];
    if (st->mc_narrow[cnt_m]) k.narrow |= 1u << 31;
  }
  for (size_t sl = 1; sl < P->slot_kind.size(); ++sl) {
    const int col = P->slot_tcol[sl];
    int m = -1;
    switch (P->slot_kind[sl]) {
      case SLOT_SUM_I64: case SLOT_SUM_F64:
        m = st->pair(PGPU_AGG_SUM, col);
        if (m < 0) m = st->pair(PGPU_AGG_AVG, col);
        break;
      case SLOT_MIN_KEY: m = st->pair(PGPU_AGG_MIN, col); break;
      default: m = st->pair(PGPU_AGG_MAX, col); break;
    }
    if (m < 0 || !st->d_mf[m]) return 0;
    k.src_f[sl] = st->d_mf[m];
    if (st->mf_narrow[m]) k.narrow |= 1u << sl;
  }
  // predicate dims: AND of the composites' matching dictIds; always-true composites are dropped
  std::vector<std::vector<uint32_t>> match(st->num_dims);
  std::vector<uint32_t> cw, lw;
  for (const auto& comp : comps) {
    const int col = q->predicates[comp[0]].column;
    const int d = st->dim_of(col);
    const int32_t card = s->cols[col].card;
    const size_t nw = ((size_t)card + 31) / 32;
    cw.assign(nw, 0u);
    for (int l : comp) {
      leaf_bitset(leaves[l], card, lw);
      for (size_t i = 0; i < nw; ++i) cw[i] |= lw[i];
    }
    int64_t ones = 0;
    for (uint32_t x : cw) ones += __builtin_popcount(x);
    if (ones == card) continue;  // isAlwaysTrue: not a predicate column for the traversal
    if (match[d].empty()) match[d].assign(nw, ~0u);
    for (size_t i = 0; i < nw; ++i) match[d][i] &= cw[i];
    k.pred_mask |= 1 << d;
  }
  *used = true;
  for (int d = 0; d < st->num_dims; ++d) {
    if (!(k.pred_mask & (1 << d))) continue;
    int64_t ones = 0;
    for (uint32_t x : match[d]) ones += __builtin_popcount(x);
    if (ones == 0) return 0;  // no matching dictId: the traversal returns null (empty result for the segment)
  }
  for (size_t j = 0; j < P->key_cols.size(); ++j) {
    const int c = P->key_cols[j];
    // K6 always gathers through the LUT (the planned version, taken under the table mutex)
    k.key_lut[j] = reinterpret_cast<const int32_t*>(P->refs->luts[seg_index * P->key_cols.size() + j]->p);
    k.key_dim[j] = st->dim_of(c);
    k.dim_card[k.key_dim[j]] = s->cols[c].card;
    if (!(k.pred_mask & (1 << k.key_dim[j]))) k.group_mask |= 1 << k.key_dim[j];
  }
  for (const auto& comp : comps) {
    const int col = q->predicates[comp[0]].column;
    k.dim_card[st->dim_of(col)] = s->cols[col].card;
  }
  {  // K6 LDS cache: the key LUTs and the match sets of the predicate dims (a superset of the residual dims)
    int64_t ints = 0;
    for (size_t j = 0; j < P->key_cols.size(); ++j) ints += k.dim_card[k.key_dim[j]];
    for (int d = 0; d < st->num_dims; ++d)
      if (k.pred_mask & (1 << d)) ints += (k.dim_card[d] + 31) / 32;
    constexpr int64_t kStarCacheMax = 8192;  // 32 KB
    if (P->star_cache_ints >= 0)
      P->star_cache_ints = ints > kStarCacheMax ? -1 : std::max<int32_t>(P->star_cache_ints, (int32_t)ints);
  }
  const int idx = (int)P->star.size();
  for (int d = 0; d < st->num_dims; ++d) {
    if (!(k.pred_mask & (1 << d))) continue;
    if (P->set_words.size() & 1) P->set_words.push_back(0);
    P->star_match_fix.emplace_back(idx, d, (int64_t)P->set_words.size());
    P->set_words.insert(P->set_words.end(), match[d].begin(), match[d].end());
  }
  const int64_t nn = st->num_nodes;
  P->star_work_off.push_back(P->star_work_bytes);
  P->star_work_bytes += ((2 * nn * 4 + (nn + 1) * 8 + 6 * nn * 4 + 8) + 15) & ~int64_t(15);
  P->star.push_back(k);
  return 0;
}


SegStats classify_segment_stats(const pgpu_plan_s* P, uint64_t sig) {
  std::vector<int32_t> lt(P->num_leaves);
  for (int l = P->num_leaves - 1; l >= 0; --l) { lt[l] = (int32_t)(sig % kStatLeafKinds); sig /= kStatLeafKinds; }
  SegStats ss;
  ss.tree = build_stat_tree(P->ops, lt);
  const StatsPlan sp = classify_stat_tree(ss.tree, 1);
  ss.kind = sp.kind;
  ss.const_per_doc = sp.constant;
  ss.range_leaves = range_index_leaves(ss.tree);
  std::vector<int> pos(P->num_leaves);  // predicate index -> evaluation position in the kernel
  for (int k = 0; k < P->num_leaves; ++k) pos[P->leaf_perm[k]] = k;
  if (sp.kind == STATS_CHAIN && P->in_kernel_stats) {
    // counted in the kernel when its evaluation order is Pinot's: index leaves, then the scans in order
    int last_idx = -1, prev_scan = -1;
    bool ok = true;
    for (int l : sp.index_leaves) last_idx = std::max(last_idx, pos[l]);
    for (int l : sp.scan_leaves) { ok &= pos[l] > last_idx && pos[l] > prev_scan; prev_scan = pos[l]; }
    if (ok) {
      ss.rec_stats = KSTATS_CHAIN;
      for (int l : sp.scan_leaves) ss.rec_stats |= 1 << (4 + pos[l]);
    } else {
      ss.kind = STATS_GENERIC;
    }
  } else if (sp.kind == STATS_LEAP2 && P->in_kernel_stats) {
    ss.rec_stats = KSTATS_LEAP2 | (pos[sp.scan_leaves[0]] << 8) | (pos[sp.scan_leaves[1]] << 10);
  } else if (sp.kind != STATS_CONST) {
    ss.kind = STATS_GENERIC;
  }
  return ss;
}

// The least and greatest integer value of a segment's column: the raw docs' range, or the ends of the sorted
// dictionary; false when it has no integer values.
bool column_int_ends(const Column& c, int64_t* lo, int64_t* hi) {
  if (c.raw) { *lo = c.raw_min; *hi = c.raw_max; return true; }
  if (c.dict.iv.empty()) return false;
  *lo = c.dict.iv.front();
  *hi = c.dict.iv.back();
  return true;
}

// The integer range of table column `col` over these segments (rt_decls.h IntRange).
IntRange int_column_range(const std::vector<Segment*>& segs, int col) {
  IntRange r;
  for (const Segment* s : segs) {
    const Column& c = s->cols[col];
    int64_t lo, hi;
    if (column_int_ends(c, &lo, &hi)) { r.lo = std::min(r.lo, lo); r.hi = std::max(r.hi, hi); }
    else if (c.dict.size() != 0) r.known = false;
  }
  return r;
}

// True when an int64 accumulator cannot overflow for SUM / AVG over integer column `col` of these segments.
bool int_sum_fits(const std::vector<Segment*>& segs, int col) { return int_sum_bound(segs, col) < 0x1p62L; }

// The bound itself: sum over segments of numDocs x max |value| (what the ranks add up when they agree on one slot
// layout, pgpu_fp_sum_range.int_sum_bound).
long double int_sum_bound(const std::vector<Segment*>& segs, int col) {
  long double bound = 0;
  for (const Segment* s : segs) {
    int64_t lo, hi;
    if (!column_int_ends(s->cols[col], &lo, &hi)) continue;
    const long double m = std::max(std::fabs((long double)lo), std::fabs((long double)hi));
    bound += m * (long double)s->num_docs;
  }
  return bound;
}

// The range of SUM / AVG operands over table column tcol that a plan of q over `segs` can read (fx_sum.h): the
// segments' dictionaries or raw docs, and the pre-aggregated doubles of the star-trees that may answer the query;
// *docs: the documents of the same segments.
FxRange fx_operand_range(pgpu_table_s* t, const std::vector<Segment*>& segs, const pgpu_query* q, int tcol,
                         int64_t* docs) {
  FxRange r;
  *docs = 0;
  std::lock_guard<std::mutex> g(t->mu);  // Column.fx is filled on first use
  for (Segment* s : segs) {
    *docs += s->num_docs;
    Column& c = s->cols[tcol];
    if (!c.fx_known) {
      if (is_int_type(c.dict.type)) for (int64_t v : c.dict.iv) fx_range_add(&c.fx, (double)v);
      else for (double v : c.dict.dv) fx_range_add(&c.fx, v);
      c.fx_known = true;
    }
    fx_range_merge(&r, c.fx);
    if (s->star && !(q->options & PGPU_OPT_NO_STAR_TREE))
      for (int fn : {PGPU_AGG_SUM, PGPU_AGG_AVG}) {
        const int m = s->star->pair(fn, tcol);
        if (m >= 0 && m < (int)s->star->mf_fx.size()) fx_range_merge(&r, s->star->mf_fx[m]);
      }
  }
  return r;
}

// pgpu_query_fp_sum_ranges: per aggregation of q what this rank reports to the agreement -- the operands' range and
// the docs exactly as a plain plan's format reads them, and int_sum_fits's own bound.
int query_fp_sum_ranges(pgpu_table_s* t, const std::vector<Segment*>& segs, const pgpu_query* q, FxAgree* out) {
  const int ncols = (int)t->names.size();
  for (int i = 0; i < q->num_aggs; ++i) {
    const pgpu_agg& a = q->aggs[i];
    out[i] = FxAgree{};
    if (a.column >= ncols && query_has_expr(t, q))
      return fail(PGPU_ERR_UNSUPPORTED, "an expression aggregation with PGPU_OPT_EXACT_FP_SUM");
    if (a.fn != PGPU_AGG_SUM && a.fn != PGPU_AGG_AVG) continue;
    if (a.column < 0 || a.column >= ncols) return fail(PGPU_ERR_INVALID_ARGUMENT, "aggregation %d: bad column", i);
    if (t->types[a.column] == PGPU_STRING) return fail(PGPU_ERR_UNSUPPORTED, "numeric aggregation over a STRING column");
    FxAgree& o = out[i];
    o.is_sum = 1;
    const FxRange r = fx_operand_range(t, segs, q, a.column, &o.docs);
    o.any = r.any ? 1 : 0;
    o.finite = r.finite ? 1 : 0;
    o.E = r.any ? r.E : 0;
    o.L = r.any ? r.L : 0;
    if (is_int_type(t->types[a.column])) o.int_sum_bound = fx_round_up(int_sum_bound(segs, a.column));
  }
  return 0;
}

// The slot whose table word also carries the COUNT (KParams.pack_slot), or -1: the first integer SUM over a column
// whose values are >= 0 in every segment, when `max_count` (the most docs one word can see) bounds both halves of the
// word -- count < 2^(64 - shift), sum < 2^shift.  Not with star-tree segments (K6 keeps its own table layout).
int32_t pack_slot_for(const pgpu_table_s* t, const pgpu_plan_s* P, const pgpu_query* q, int64_t max_count,
                      int shift) {
  if (P->slot_kind.empty() || P->slot_kind[0] != SLOT_COUNT || shift <= 0 || shift >= 64) return -1;
  if (max_count >= (INT64_C(1) << (64 - shift))) return -1;
  for (const Segment* s : P->segs)
    if (s->star && !(q->options & PGPU_OPT_NO_STAR_TREE)) return -1;
  for (size_t sl = 1; sl < P->slot_kind.size(); ++sl) {
    const int c = P->slot_tcol[sl];
    if (P->slot_kind[sl] != SLOT_SUM_I64 || c < 0 || c == kDocIdColumn || !is_int_type(t->types[c])) continue;
    if (P->slot_fx[sl] >= 0) continue;  // a fixed-point digit (of an integer column past int_sum_fits): signed
    if (P->slot_dc[sl] >= 0) continue;  // a DISTINCTCOUNT row: written after the scan, never added to
    const IntRange r = int_column_range(P->segs, c);
    if (r.known && r.lo <= r.hi && r.lo >= 0 && (long double)max_count * (long double)r.hi < ldexpl(1.0L, shift))
      return (int32_t)sl;
  }
  return -1;
}

// LDS-table plans (shift 40): a workgroup scans at most ceil(tiles / grid) + 2 tiles under either tile order, and the
// grid is at least min(tiles, CUs).
int32_t lds_pack_slot(const pgpu_table_s* t, const pgpu_plan_s* P, const pgpu_query* q, int64_t G) {
  if (G <= 1) return -1;
  int64_t tiles = 0;
  for (const Segment* s : P->segs) tiles += ((int64_t)s->num_docs + kTileDocs - 1) / kTileDocs;
  const int64_t min_grid = std::max<int64_t>(1, std::min<int64_t>(tiles, t->num_cus));
  const int64_t wg_docs = ((tiles + min_grid - 1) / min_grid + 2) * kTileDocs;
  return pack_slot_for(t, P, q, wg_docs, kLdsPackShift);
}

// Hash-table plans: one word sees at most every doc of the plan, so the COUNT takes bits(total_docs) high bits; the
// scan's adds stay packed and hash_unpack splits the occupied words after it (exec_epilogue).  Single-stage keys only.
int32_t hash_pack_slot(const pgpu_table_s* t, const pgpu_plan_s* P, const pgpu_query* q, int* shift) {
  if (!P->stage_end.empty() || P->total_docs <= 0) return -1;
  int bits = 0;
  while (bits < 63 && (INT64_C(1) << bits) <= P->total_docs) ++bits;
  *shift = 64 - bits;
  return pack_slot_for(t, P, q, P->total_docs, *shift);
}

// Hashed partitions (KPartParams.hashed) for a MODE_HASH plan: single-stage keys whose composite key fits int32
// (part_keys' arithmetic and the records' u32 keys), unless pgpu_config.hash_partitions is 0 (the global hash table).
bool part_hash_eligible(const pgpu_plan_s* P, int64_t G) {
  return P->cfg.hash_partitions && P->mode == MODE_HASH && P->stage_end.empty() && G > 0 && G < (INT64_C(1) << 31) && P->key_bias == 0;
}

// Dense partitions (partition.h) for a MODE_GLOBAL plan: tables of at least kPartMinBytes.
bool dense_part_eligible(const pgpu_plan_s* P, int nslots, int64_t G) {
  return P->mode == MODE_GLOBAL && (int64_t)nslots * G * 8 >= kPartMinBytes;
}

// Either kind, unless pgpu_config.partitioned_group_by is 0.
bool part_eligible(const pgpu_plan_s* P, int nslots, int64_t G) {
  return (dense_part_eligible(P, nslots, G) || part_hash_eligible(P, G)) && P->cfg.partitioned_group_by;
}

// Hashed partitions' shape for `groups` expected groups: 2^pbits partitions (K8a / K8c's LDS histogram: at most
// kMaxParts) of LDS hash tables of 2^sbits entries (4 + 8 x slots bytes each).  Small tables keep more K8h
// workgroups on a CU, so the tables are 2^10 entries at a load of at most ~0.6 and partitions are added first; past
// kMaxParts partitions the tables grow, up to kHashPartLdsMax (more groups than that take further K8h rounds).
// Measured on c5_hash (10^7 groups, r04, ms per query): 2^14 x 2^10 (20 KB) 3.69-3.72, 2^13 x 2^11 (40 KB)
// 4.06-4.17, 2^13 x 2^12 (80 KB) 7.67, 2^14 x 2^12 11.7-12.7; the global hash table 14.8.  pgpu_config's
// hash_partition_lds_kb / hash_partition_bits (tests force K8h's extra rounds with them) cap the table bytes and the
// partition bits.
void hash_part_bits(const pgpu_config& cfg, int64_t groups, int nslots, int* pbits, int* sbits) {
  const int64_t lds_cap = cfg.hash_partition_lds_kb > 0
                              ? std::min<int64_t>((int64_t)cfg.hash_partition_lds_kb * 1024, 128 * 1024)
                              : kHashPartLdsMax;
  const int max_pbits = std::max(0, std::min(14, cfg.hash_partition_bits));
  auto fits = [&](int p, int sb) { return (long double)groups <= 0.6L * (long double)(int64_t(1) << (p + sb)); };
  int sb = 10;
  while (sb > 8 && (int64_t)part_hash_lds(sb, nslots) > lds_cap) --sb;
  int p = 0;
  while (p < max_pbits && !fits(p, sb)) ++p;
  while (!fits(p, sb) && sb < 14 && (int64_t)part_hash_lds(sb + 1, nslots) <= lds_cap) ++sb;
  *pbits = p;
  *sbits = sb;
}

// Coarse runs of the two-level scatter: 2^cshift consecutive partitions each, at most 64 (KPartParams.cshift).
int part_coarse_shift(int num_parts) {
  int cshift = 0;
  while ((num_parts + (1 << cshift) - 1) >> cshift > 64) ++cshift;
  return cshift;
}
int part_coarse_runs(int num_parts) {
  const int cshift = part_coarse_shift(num_parts);
  return (num_parts + (1 << cshift) - 1) >> cshift;
}

// The partition pass kernels' LDS (the partition histogram, and the filter stack of general programs) and grid for
// `parts` partitions over `tiles` tiles: P->part_lds and P->part_grid.  False, and neither set, past the passes' 96 KB.
bool part_pass_shape(pgpu_plan_s* P, int64_t parts, int64_t tiles) {
  const size_t pass_lds = (size_t)((parts + 3) & ~int64_t(3)) * 4 + (P->pure_and ? 0 : (size_t)kMaxStack * kBlock * 4);
  if (pass_lds > 96 * 1024) return false;
  P->part_lds = pass_lds;
  int per_cu = occupancy_part_pass(pass_lds, (int)parts, part_coarse_runs((int)parts), 0);
  per_cu = std::max(1, std::min(per_cu, 4));
  P->part_grid = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)P->table->num_cus * per_cu));
  return true;
}

// A cached hashed-partition plan re-shaped for the groups its last execution found (plan_cache_get): the partition
// count, the pass kernels' LDS and grid follow.
void hash_part_resize(pgpu_plan_s* P, int64_t groups) {
  int pbits = 0, sbits = 0;
  hash_part_bits(P->cfg, groups, (int)P->slot_kind.size(), &pbits, &sbits);
  if (!part_pass_shape(P, int64_t(1) << pbits, P->num_tiles)) return;
  P->part_pbits = pbits;
  P->part_sbits = sbits;
  P->num_parts = 1 << pbits;
  P->part_grid_staged[0] = P->part_grid_staged[1] = 0;
}

// Records K8h may append (the groups): as finalize's compaction of a hash table sizes its output.
int64_t part_hash_out_cap(const pgpu_plan_s* P) {
  return std::max<int64_t>(1, std::min<int64_t>(P->num_keys, std::max<int64_t>(P->total_docs, 1)));
}

// K8h found more groups than its record buffer holds (the bound above is exact for the plan's key space and docs, so
// this is a planning bug, reported instead of a truncated result)
int part_hash_overflow(const pgpu_plan_s* P, uint64_t groups) {
  return fail(PGPU_ERR_DEVICE, "hashed partitions found %llu groups, past their record buffer of %lld",
              (unsigned long long)groups, (long long)part_hash_out_cap(P));
}

}  // namespace pgpu
