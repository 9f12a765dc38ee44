// expr_filter_check.cpp -- host check of the expression filter leaves (WHERE price * qty > 1000): the task builder and
// job list of pinot_amd/csrc/expr_leaf.h and the ExpressionScanDocIdIterator replay of filter_stats.cpp (SL_EXPR /
// IT_EXPR).  A stand-alone program built under AddressSanitizer + UndefinedBehaviorSanitizer by
// pinot_amd.build.build_expr_filter_check (this file and filter_stats.cpp; no device code, no library) and run by
// tests/test_expr_filter_cpu.py.  Prints "expr_filter_check: ok" and exits 0, or the first failed check and exits 1.
//
// What it checks:
//   - a task built from a program and a translated predicate carries the operands, bounds / key-set range, negate and
//     destination; the IN keys of several tasks are appended back to back;
//   - the jobs of a task list cover every doc of every task exactly once, and a host restatement of the kernel's walk
//     over the same task -- gather, evaluate (expr_eval), key, test, negate, bits past numDocs clear, both words of
//     every 64-doc pair stored -- stays inside each task's region of leaf_region_words words and gives the bits worked
//     out doc by doc (this is evidence about the host's task, jobs and regions; the kernel's own code runs in the GPU
//     tests only);
//   - simulate_entries_scanned with expression leaves against counts worked out by hand (the 36006 anchor, a lone
//     leaf, an OR, applyAnd after an index leaf, blocks that start at advance() targets, blocks without a match).
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "expr_leaf.h"
#include "filter_stats.h"
#include "host_common.h"

// filter_stats.cpp reports through the runtime's error helpers, which live in translation units that need the device
// runtime; the check has its own.
namespace pgpu {
int host_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  return code;
}
int abi_exception() noexcept { return -1; }
}  // namespace pgpu

namespace {

using namespace pgpu;

int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      g_failed = 1;                                                         \
    }                                                                       \
  } while (0)

// A column as the kernel reads it: MSB-first fixed-bit dictIds in big-endian u32 words (padded like a pinned column)
// and its dictId -> double table.
struct HostColumn {
  int bits = 0;
  std::vector<uint32_t> fwd;
  std::vector<double> dval;
  std::vector<uint32_t> ids;
};

// What expr_operands (expr_eval.h) reads of a segment: its columns' device arrays, here the host's.
struct HostSegment {
  struct Col {
    const uint32_t* d_fwd = nullptr;
    const double* d_val = nullptr;
    int32_t bits = 0;
  };
  std::vector<Col> cols;
};

uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

HostColumn make_column(int bits, const std::vector<double>& values, int32_t num_docs, uint64_t seed) {
  HostColumn c;
  c.bits = bits;
  c.dval = values;
  c.ids.resize((size_t)num_docs);
  const size_t words = ((size_t)num_docs * bits + 31) / 32 + kFwdPadWords;
  std::vector<uint32_t> be(words, 0);
  for (int32_t d = 0; d < num_docs; ++d) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t id = (uint32_t)((seed >> 33) % values.size());
    c.ids[(size_t)d] = id;
    for (int b = 0; b < bits; ++b) {
      const uint64_t bit = (uint64_t)d * bits + b;
      if ((id >> (bits - 1 - b)) & 1u) be[bit >> 5] |= 1u << (31 - (bit & 31));
    }
  }
  c.fwd.resize(words);
  for (size_t i = 0; i < words; ++i) c.fwd[i] = bswap(be[i]);  // memory holds the big-endian bytes
  return c;
}

// device.h gather_id on the host.
uint32_t gather_id(const uint32_t* fwd, int bits, int64_t doc) {
  const uint64_t bit = (uint64_t)doc * (uint64_t)bits;
  const uint64_t wi = bit >> 5;
  const uint32_t sh = (uint32_t)(bit & 31);
  const uint64_t two = ((uint64_t)bswap(fwd[wi]) << 32) | (uint64_t)bswap(fwd[wi + 1]);
  return (uint32_t)(two >> (64 - sh - bits)) & ((1u << bits) - 1u);
}

// expr_leaf_bitmap_kernel's steps for one job restated on the host, in the kernel's order -- per wave four 64-doc steps
// per iteration, the IN test a binary search of the sorted key set -- with every store bounds-checked against the
// task's region.  A restatement, not the kernel: it shows that the task, the job list and the region arithmetic fit
// that walk; the kernel's own loop and search are covered by the GPU tests alone.
void run_job(const KExprLeafJob& J, const std::vector<KExprLeafTask>& tasks, const std::vector<int64_t>& vals,
             std::vector<uint32_t>& docbits, std::vector<int32_t>& seen) {
  const KExprLeafTask& T = tasks[(size_t)J.task];
  const int64_t region = leaf_region_words(T.num_docs);
  constexpr int kWaveDocs = kExprLeafJobDocs / 4, kU = 4;
  for (int wave = 0; wave < 4; ++wave)
    for (int it = 0; it < kWaveDocs / (64 * kU); ++it) {
      const int64_t base = (int64_t)J.doc0 + wave * kWaveDocs + it * (64 * kU);
      if (base >= T.num_docs) break;
      for (int u = 0; u < kU; ++u) {
        const int64_t d0 = base + u * 64;
        if (d0 >= T.num_docs) break;
        uint64_t m = 0;
        for (int lane = 0; lane < 64; ++lane) {
          const int64_t doc = d0 + lane;
          if (doc >= T.num_docs) continue;
          seen[(size_t)doc]++;
          double v[kExprMaxCols][1] = {{0.0}, {0.0}, {0.0}, {0.0}}, out[1];
          for (int c = 0; c < T.prog.ncols; ++c) v[c][0] = T.ops.dval[c][gather_id(T.ops.fwd[c], T.ops.bits[c], doc)];
          expr_eval<1>(T.prog, v, out);
          const int64_t key = expr_value_key(out[0]);
          bool hit;
          if (T.kind == LEAF_RAW_RANGE) {
            hit = T.lo <= key && key <= T.hi;
          } else {
            CHECK(T.lo >= 0 && T.lo + T.hi <= (int64_t)vals.size());
            const int64_t* set = vals.data() + T.lo;
            const int n = (int)T.hi;
            int a = 0, b = n;  // first set key >= key
            while (a < b) {
              const int mid = (a + b) >> 1;
              if (set[mid] < key) a = mid + 1;
              else b = mid;
            }
            hit = a < n && set[a] == key;
          }
          if (T.negate) hit = !hit;
          if (hit) m |= 1ull << lane;
        }
        const int64_t w = d0 >> 5;
        CHECK(w + 1 < region);
        docbits.at((size_t)(T.dst + w)) = (uint32_t)m;
        docbits.at((size_t)(T.dst + w + 1)) = (uint32_t)(m >> 32);
      }
    }
}

void check_tasks() {
  const int32_t docs[] = {1, 63, 64, 70, 8191, 8192, 8193, 25003};
  // price * qty - 3.5 / x: three columns of 1-, 5- and 11-bit dictIds
  const ExprOpIn ops[] = {{EXPR_COLUMN, 7, 0.0}, {EXPR_COLUMN, 2, 0.0}, {EXPR_MULT, 0, 0.0}, {EXPR_LITERAL, 0, 3.5},
                          {EXPR_COLUMN, 9, 0.0}, {EXPR_DIV, 0, 0.0},    {EXPR_SUB, 0, 0.0}};
  ExprProg prog;
  CHECK(expr_compile(ops, 7, &prog) == EXPR_OK);
  CHECK(prog.ncols == 3 && prog.col[0] == 7 && prog.col[1] == 2 && prog.col[2] == 9);
  std::vector<KExprLeafTask> tasks;
  std::vector<int64_t> vals;
  std::vector<std::vector<HostColumn>> cols;
  int64_t words = 0;
  for (size_t s = 0; s < sizeof docs / sizeof docs[0]; ++s) {
    std::vector<double> v1 = {-2.0, 0.0}, v5, v11;
    for (int i = 0; i < 20; ++i) v5.push_back(i * 0.25 - 1.0);
    for (int i = 0; i < 2000; ++i) v11.push_back(i == 0 ? 0.0 : i * 0.5 - 100.0);  // 0.0: a division by zero
    cols.push_back({make_column(1, v1, docs[s], 11 + s), make_column(5, v5, docs[s], 23 + s),
                    make_column(11, v11, docs[s], 37 + s)});
  }
  for (size_t s = 0; s < cols.size(); ++s) {
    HostSegment seg;  // the program's operands are its columns 7, 2 and 9, filled as the planner fills a task's
    seg.cols.resize(10);
    for (int c = 0; c < 3; ++c)
      seg.cols[(size_t)prog.col[c]] = {cols[s][(size_t)c].fwd.data(), cols[s][(size_t)c].dval.data(), cols[s][(size_t)c].bits};
    const ExprOperands o = expr_operands(seg, prog);
    const bool in = s % 2 == 1;
    const std::vector<int64_t> raw = in ? std::vector<int64_t>{expr_value_key(-0.0), expr_value_key(0.0), expr_value_key(1.5)}
                                        : std::vector<int64_t>{expr_value_key(-1.0), expr_value_key(1e300)};
    const size_t before = vals.size();
    tasks.push_back(make_expr_leaf_task(prog, o, docs[s], in, raw, (int)(s % 3 == 0), words, 0, &vals));
    const KExprLeafTask& t = tasks.back();
    CHECK(t.num_docs == docs[s] && t.dst == words && t.negate == (s % 3 == 0));
    CHECK(t.ops.fwd[2] == cols[s][2].fwd.data() && t.ops.dval[1] == cols[s][1].dval.data() && t.ops.bits[0] == 1 &&
          t.ops.bits[2] == 11 && t.ops.fwd[3] == nullptr);
    if (in) CHECK(t.kind == LEAF_RAW_IN && t.lo == (int64_t)before && t.hi == 3 && vals.size() == before + 3);
    else CHECK(t.kind == LEAF_RAW_RANGE && t.lo == raw[0] && t.hi == raw[1] && vals.size() == before);
    words += leaf_region_words(docs[s]);
  }
  std::vector<KExprLeafJob> jobs;
  expr_leaf_jobs(tasks, &jobs);
  std::vector<uint32_t> docbits((size_t)words, 0xdeadbeefu);
  std::vector<std::vector<int32_t>> seen;
  for (const KExprLeafTask& t : tasks) seen.emplace_back((size_t)t.num_docs, 0);
  for (const KExprLeafJob& j : jobs) {
    CHECK(j.task >= 0 && j.task < (int32_t)tasks.size() && j.doc0 >= 0 && j.doc0 < tasks[(size_t)j.task].num_docs);
    CHECK(j.doc0 % kExprLeafJobDocs == 0);
    run_job(j, tasks, vals, docbits, seen[(size_t)j.task]);
  }
  for (size_t s = 0; s < tasks.size(); ++s) {
    const KExprLeafTask& t = tasks[s];
    for (int32_t d = 0; d < t.num_docs; ++d) CHECK(seen[s][(size_t)d] == 1);
    for (int64_t w = 0; w < leaf_region_words(t.num_docs); ++w) CHECK(docbits[(size_t)(t.dst + w)] != 0xdeadbeefu);
    // against the values worked out doc by doc from the dictIds
    for (int32_t d = 0; d < t.num_docs; ++d) {
      const double a = cols[s][0].dval[cols[s][0].ids[(size_t)d]], b = cols[s][1].dval[cols[s][1].ids[(size_t)d]];
      const double x = cols[s][2].dval[cols[s][2].ids[(size_t)d]];
      const double want = expr_apply(EXPR_SUB, expr_apply(EXPR_MULT, a, b), expr_apply(EXPR_DIV, 3.5, x));
      const int64_t key = expr_value_key(want);
      bool hit = t.kind == LEAF_RAW_RANGE ? (t.lo <= key && key <= t.hi) : false;
      if (t.kind == LEAF_RAW_IN)
        for (int64_t i = 0; i < t.hi; ++i) hit |= vals[(size_t)(t.lo + i)] == key;
      if (t.negate) hit = !hit;
      CHECK(((docbits[(size_t)(t.dst + (d >> 5))] >> (d & 31)) & 1u) == (hit ? 1u : 0u));
    }
    for (int64_t d = t.num_docs; d < leaf_region_words(t.num_docs) * 32; ++d)  // bits past numDocs clear
      CHECK(((docbits[(size_t)(t.dst + (d >> 5))] >> (d & 31)) & 1u) == 0u);
  }
  // an empty range (no bounds) matches nothing
  const ExprOperands o = {};
  std::vector<int64_t> none;
  const KExprLeafTask e = make_expr_leaf_task(prog, o, 5, false, {1, 0}, 0, 0, 0, &none);
  CHECK(e.lo > e.hi && none.empty());
}

std::vector<uint32_t> words_of(const std::vector<uint8_t>& m) {
  std::vector<uint32_t> w((m.size() + 31) / 32, 0u);
  for (size_t d = 0; d < m.size(); ++d)
    if (m[d]) w[d >> 5] |= 1u << (d & 31);
  return w;
}

int64_t entries(const std::vector<int32_t>& ops, const std::vector<int32_t>& types,
                const std::vector<std::vector<uint8_t>>& masks) {
  std::vector<std::vector<uint32_t>> w;
  for (const auto& m : masks) w.push_back(words_of(m));
  std::vector<const uint32_t*> p;
  for (const auto& x : w) p.push_back(x.data());
  return simulate_entries_scanned(build_stat_tree(ops, types), p, (int32_t)masks[0].size());
}

int32_t leaf(int i) { return (OP_LEAF << 16) | i; }
int32_t op_and(int n) { return (OP_AND << 16) | n; }
int32_t op_or(int n) { return (OP_OR << 16) | n; }

void check_replay() {
  const int32_t n = 25003;
  std::vector<uint8_t> all((size_t)n, 1), two((size_t)n, 0), none_after((size_t)n, 0), first_half((size_t)n, 0);
  two[12345] = two[24000] = 1;
  for (int32_t d = 0; d < 12000; ++d) first_half[(size_t)d] = 1;
  none_after[3] = 1;
  // the anchor: AND(scan, expr), either way round
  CHECK(entries({leaf(0), leaf(1), op_and(2)}, {SL_SCAN, SL_EXPR}, {two, all}) == 36006);
  CHECK(entries({leaf(0), leaf(1), op_and(2)}, {SL_EXPR, SL_SCAN}, {all, two}) == 36006);
  // a lone leaf and an OR: numDocs per expression leaf, whatever matches
  CHECK(entries({leaf(0)}, {SL_EXPR}, {two}) == n);
  CHECK(entries({leaf(0)}, {SL_EXPR}, {none_after}) == n);
  CHECK(entries({leaf(0), leaf(1), op_or(2)}, {SL_EXPR, SL_SCAN}, {two, all}) == 2 * (int64_t)n);
  CHECK(entries({leaf(0), leaf(1), op_or(2)}, {SL_EXPR, SL_BITMAP}, {two, first_half}) == n);
  // applyAnd after an index leaf: the index leaf's docs, then what the scan left
  CHECK(entries({leaf(0), leaf(1), op_and(2)}, {SL_EXPR, SL_BITMAP}, {two, first_half}) == 12000);
  CHECK(entries({leaf(0), leaf(1), leaf(2), op_and(3)}, {SL_EXPR, SL_SCAN, SL_SORTED}, {all, two, first_half}) == 12000);
  // AND(expr, expr): the first runs block after block; the second starts blocks at the first's docs
  //   first = {12345, 24000}: blocks [0,10000) [10000,20000) -> 12345; second (all) evaluates [12345,22345);
  //   then first advances to 12346: inside its block, uncounted, nothing there -> [20000,25003) -> 24000; second
  //   evaluates [24000,25003); then first advances to 24001: in block, nothing, no block left -> EOF
  CHECK(entries({leaf(0), leaf(1), op_and(2)}, {SL_EXPR, SL_EXPR}, {two, all}) == (20000 + 5003) + (10000 + 1003));
  // a block without a match is counted and the next one follows it
  std::vector<uint8_t> late((size_t)n, 0);
  late[24999] = 1;
  //   scan = {3}: docs 0..3, then -- the expression answering 24999 -- docs 24999..EOF; expr: blocks from 3 to the end
  CHECK(entries({leaf(0), leaf(1), op_and(2)}, {SL_SCAN, SL_EXPR}, {none_after, late}) == (4 + 4) + (int64_t)(n - 3));
  // classification: never the leap-frog kernel count, the chain with the expression leaves last
  StatsPlan p = classify_stat_tree(build_stat_tree({leaf(0), leaf(1), op_and(2)}, {SL_EXPR, SL_SCAN}), n);
  CHECK(p.kind == STATS_GENERIC);
  p = classify_stat_tree(build_stat_tree({leaf(0), leaf(1), leaf(2), op_and(3)}, {SL_EXPR, SL_SCAN, SL_BITMAP}), n);
  CHECK(p.kind == STATS_CHAIN && p.index_leaves == std::vector<int32_t>{2} && (p.scan_leaves == std::vector<int32_t>{1, 0}));
  p = classify_stat_tree(build_stat_tree({leaf(0), leaf(1), op_or(2)}, {SL_EXPR, SL_EXPR}), n);
  CHECK(p.kind == STATS_CONST && p.constant == 2 * (int64_t)n);
  p = classify_stat_tree(build_stat_tree({leaf(0)}, {SL_EXPR}), n);
  CHECK(p.kind == STATS_CONST && p.constant == n);
  p = classify_stat_tree(build_stat_tree({leaf(0), leaf(1), op_and(2)}, {SL_SCAN, SL_SCAN}), n);
  CHECK(p.kind == STATS_LEAP2);  // (as before)
}

}  // namespace

int main() {
  check_tasks();
  check_replay();
  if (g_failed) return 1;
  printf("expr_filter_check: ok\n");
  return 0;
}
