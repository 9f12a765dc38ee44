// math_check.cpp -- host check of the math and time ops of the expression programs (pinot_amd/csrc/expr_eval.h: ABS,
// CEIL, FLOOR, SQRT, MOD, LDIV; nothing else of the library is included or linked).  Built under AddressSanitizer +
// UndefinedBehaviorSanitizer with floating-point contraction off by pinot_amd.build.build_math_check, run by
// tests/test_time_expr_cpu.py.  It takes no input and checks, bit for bit:
//   1. every new op over the edge values (+-0.0, halves, +-inf, NaN, squares, the ends of the doubles) against libm and
//      the values Java documents for them;
//   2. LDIV against plain int64_t division, for dividends at +-(2^53 - 1), +-2^53 and around every multiple of the
//      divisor that matters (the first ones of both signs and the last ones within +-2^53), and for random pairs;
//   3. random programs holding the new ops (compiled by expr_compile, run by expr_eval) against a direct evaluation of
//      the tree they were emitted from.
// Output: one "ok <what> <count>" line per part; any mismatch is printed and makes the exit status 1.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "expr_eval.h"

namespace {

using namespace pgpu;

int g_bad = 0;

uint64_t bits(double d) { return (uint64_t)bits_of_double(d); }
// (a NaN's payload and sign are the machine's: the key is what the library compares)
bool same(double a, double b) { return a != a ? b != b : bits(a) == bits(b); }

void expect(bool ok, const char* what, double a, double b, double got, double want) {
  if (ok) return;
  ++g_bad;
  printf("MISMATCH %s(%.17g [%016" PRIx64 "], %.17g): got %.17g [%016" PRIx64 "], want %.17g [%016" PRIx64 "]\n", what, a,
         bits(a), b, got, bits(got), want, bits(want));
}

// One stack operation through the evaluator's own dispatch: s1 op s0 (s0 alone for a unary op).
double stack_op(int op, double a, double b) {
  const bool unary = op >= EXPR_ABS && op <= EXPR_SQRT;
  double s0[1] = {unary ? a : b}, s1[1] = {unary ? 5.0 : a}, s2[1] = {7.0}, s3[1] = {9.0};
  expr_stack_op<1>(op, s0, s1, s2, s3);
  // the rows below: untouched by a unary op, shifted down by a binary one
  if (unary ? (s1[0] != 5.0 || s2[0] != 7.0) : (s1[0] != 7.0 || s2[0] != 9.0)) {
    ++g_bad;
    printf("MISMATCH op %d moved the stack wrongly\n", op);
  }
  return s0[0];
}

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

int check_edges() {
  const double edge[] = {0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1.0, -1.0, 2.0, 3.0, 4.0, -4.0, 9.0, 10.0, 1e-310, -1e-310,
                         5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 4503599627370496.5, 9007199254740992.0,
                         -9007199254740991.0, 0.99999999999999989, -0.99999999999999989, 7.0, -7.0, 1e22, kInf, -kInf, kNaN};
  int n = 0;
  for (double a : edge) {
    expect(same(stack_op(EXPR_ABS, a, 0), std::fabs(a)), "abs", a, 0, stack_op(EXPR_ABS, a, 0), std::fabs(a)), ++n;
    expect(same(stack_op(EXPR_CEIL, a, 0), std::ceil(a)), "ceil", a, 0, stack_op(EXPR_CEIL, a, 0), std::ceil(a)), ++n;
    expect(same(stack_op(EXPR_FLOOR, a, 0), std::floor(a)), "floor", a, 0, stack_op(EXPR_FLOOR, a, 0), std::floor(a)), ++n;
    expect(same(stack_op(EXPR_SQRT, a, 0), std::sqrt(a)), "sqrt", a, 0, stack_op(EXPR_SQRT, a, 0), std::sqrt(a)), ++n;
    for (double b : edge)
      expect(same(stack_op(EXPR_MOD, a, b), std::fmod(a, b)), "mod", a, b, stack_op(EXPR_MOD, a, b), std::fmod(a, b)), ++n;
  }
  // what Java documents (Math.abs / ceil / floor / sqrt, JLS 15.17.3 for %), stated on their own
  struct { int op; double a, b; uint64_t want; } kat[] = {
      {EXPR_ABS, -0.0, 0, 0x0000000000000000ull},   {EXPR_ABS, -kInf, 0, 0x7ff0000000000000ull},
      {EXPR_CEIL, -0.5, 0, 0x8000000000000000ull},  {EXPR_CEIL, 0.5, 0, 0x3ff0000000000000ull},
      {EXPR_CEIL, -0.0, 0, 0x8000000000000000ull},  {EXPR_FLOOR, -0.5, 0, 0xbff0000000000000ull},
      {EXPR_FLOOR, 0.5, 0, 0x0000000000000000ull},  {EXPR_FLOOR, -0.0, 0, 0x8000000000000000ull},
      {EXPR_SQRT, -0.0, 0, 0x8000000000000000ull},  {EXPR_SQRT, 4.0, 0, 0x4000000000000000ull},
      {EXPR_SQRT, 2.0, 0, 0x3ff6a09e667f3bcdull},   {EXPR_SQRT, kInf, 0, 0x7ff0000000000000ull},
      {EXPR_MOD, -7.0, 3.0, 0xbff0000000000000ull}, {EXPR_MOD, 7.0, -3.0, 0x3ff0000000000000ull},
      {EXPR_MOD, -6.0, 3.0, 0x8000000000000000ull}, {EXPR_MOD, 5.5, kInf, 0x4016000000000000ull},
      {EXPR_MOD, 5.5, 2.0, 0x3ff8000000000000ull},  {EXPR_LDIV, -1.0, 86400000.0, 0x0000000000000000ull},
      {EXPR_LDIV, -86400000.0, 86400000.0, 0xbff0000000000000ull}, {EXPR_LDIV, -86400001.0, 86400000.0, 0xbff0000000000000ull},
      {EXPR_LDIV, 86399999.0, 86400000.0, 0x0000000000000000ull}};
  for (const auto& k : kat) {
    const double got = stack_op(k.op, k.a, k.b);
    double want;
    memcpy(&want, &k.want, 8);
    expect(bits(got) == k.want, "known answer", k.a, k.b, got, want), ++n;
  }
  for (double a : {-1.0, -kInf, kNaN}) expect(stack_op(EXPR_SQRT, a, 0) != stack_op(EXPR_SQRT, a, 0), "sqrt is NaN", a, 0, 0, kNaN), ++n;
  for (double a : {1.0, 0.0, kInf, -kInf, kNaN}) {
    expect(stack_op(EXPR_MOD, a, 0.0) != stack_op(EXPR_MOD, a, 0.0), "x % 0 is NaN", a, 0, 0, kNaN), ++n;
    expect(stack_op(EXPR_MOD, kInf, a) != stack_op(EXPR_MOD, kInf, a), "inf % y is NaN", kInf, a, 0, kNaN), ++n;
  }
  return n;
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

constexpr int64_t kExact = 1ll << 53;

void ldiv_case(int64_t a, int64_t b, int* n) {
  if (a < -kExact || a > kExact || b < 1 || b > kExact) return;
  const double got = stack_op(EXPR_LDIV, (double)a, (double)b), want = (double)(a / b);
  expect(bits(got) == bits(want), "ldiv", (double)a, (double)b, got, want);
  ++*n;
}

int check_ldiv() {
  const int64_t divisors[] = {1, 2, 3, 7, 10, 60, 1000, 3600, 86400, 900000, 1000000, 3600000, 86400000, 604800000,
                              86400000000000ll, (1ll << 26) + 1, (1ll << 27) - 1, (1ll << 52) + 1, kExact - 1, kExact};
  int n = 0;
  for (int64_t b : divisors) {
    for (int64_t a : {(int64_t)0, (int64_t)1, (int64_t)-1, kExact - 1, -(kExact - 1), kExact, -kExact, kExact - 2, -(kExact - 2)})
      ldiv_case(a, b, &n);
    const int64_t last = kExact / b;  // the last multiple within 2^53
    for (int64_t k : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)1000, last - 2, last - 1, last, last / 2, last / 3})
      for (int64_t off : {-2, -1, 0, 1, 2})
        for (int sign : {1, -1}) {
          if (k < 0 || (k > 0 && k > kExact / b)) continue;
          ldiv_case(sign * (k * b + off), b, &n);
        }
  }
  for (int i = 0; i < 400000; ++i) {
    const int64_t a = (int64_t)(rnd() >> (10 + rnd() % 44)) * ((rnd() & 1) ? 1 : -1);
    const int64_t b = (int64_t)(rnd() >> (11 + rnd() % 53)) + 1;
    ldiv_case(a, b, &n);
    // ... and a dividend right at a multiple of a random divisor, where the rounded quotient is an integer too early
    const int64_t k = b > 0 ? (int64_t)(rnd() % (uint64_t)(kExact / b + 1)) : 0;
    ldiv_case(k * b - 1, b, &n);
    ldiv_case(-(k * b - 1), b, &n);
  }
  return n;
}

// ---- random programs against the trees they come from
struct Node {
  int op;  // an ExprOpCode; EXPR_COLUMN uses col, EXPR_LITERAL uses lit
  int col = 0;
  double lit = 0.0;
  std::unique_ptr<Node> a, b;
};

std::unique_ptr<Node> leaf_col(int c) {
  auto n = std::make_unique<Node>();
  n->op = EXPR_COLUMN;
  n->col = c;
  return n;
}
std::unique_ptr<Node> leaf_lit(double v) {
  auto n = std::make_unique<Node>();
  n->op = EXPR_LITERAL;
  n->lit = v;
  return n;
}
std::unique_ptr<Node> node(int op, std::unique_ptr<Node> a, std::unique_ptr<Node> b = nullptr) {
  auto n = std::make_unique<Node>();
  n->op = op;
  n->a = std::move(a);
  n->b = std::move(b);
  return n;
}

// An integral value: columns 0 and 1 hold integers of magnitude below 2^30; *bound is the greatest magnitude so far, kept
// within 2^53 -- the precondition the plan checks.
std::unique_ptr<Node> gen_int(int level, int64_t* bound) {
  const int pick = level <= 0 ? 0 : (int)(rnd() % 3);
  if (pick == 0) {
    *bound = 1ll << 30;
    return leaf_col((int)(rnd() & 1));
  }
  auto x = gen_int(level - 1, bound);
  const int64_t consts[] = {1, 2, 7, 60, 1000, 86400, 3600000, 86400000, 604800000};
  const int64_t n = consts[rnd() % 9];
  if (pick == 1 && *bound <= kExact / n) {
    *bound *= n;
    return node(EXPR_MULT, std::move(x), leaf_lit((double)n));
  }
  return node(EXPR_LDIV, std::move(x), leaf_lit((double)n));
}

std::unique_ptr<Node> gen_num(int level) {
  const int pick = level <= 0 ? (int)(rnd() % 2) : (int)(rnd() % 9);
  if (pick == 0) return leaf_col((int)(rnd() % 4));
  if (pick == 1) {
    const double lits[] = {0.0, -0.0, 0.5, -2.5, 3.0, 7.0, -7.0, 10.0, 1e-3, 86400.0};
    return level <= 0 ? leaf_col((int)(rnd() % 4)) : leaf_lit(lits[rnd() % 10]);
  }
  if (pick <= 3) return node(EXPR_ADD + (int)(rnd() % 4), gen_num(level - 1), gen_num(level - 1));
  if (pick <= 5) return node(EXPR_ABS + (int)(rnd() % 4), gen_num(level - 1));
  if (pick <= 6) return node(EXPR_MOD, gen_num(level - 1), gen_num(level - 1));
  int64_t bound = 0;
  return gen_int(level, &bound);
}

void emit(const Node& n, std::vector<ExprOpIn>* ops) {
  if (n.a) emit(*n.a, ops);
  if (n.b) emit(*n.b, ops);
  ops->push_back(ExprOpIn{n.op, n.col, n.lit});
}

// The tree evaluated as written: C++'s own operators, libm, and int64_t division for LDIV.
double direct(const Node& n, const double* v) {
  switch (n.op) {
    case EXPR_COLUMN: return v[n.col];
    case EXPR_LITERAL: return n.lit;
    case EXPR_ADD: return direct(*n.a, v) + direct(*n.b, v);
    case EXPR_SUB: return direct(*n.a, v) - direct(*n.b, v);
    case EXPR_MULT: return direct(*n.a, v) * direct(*n.b, v);
    case EXPR_DIV: return direct(*n.a, v) / direct(*n.b, v);
    case EXPR_ABS: return std::fabs(direct(*n.a, v));
    case EXPR_CEIL: return std::ceil(direct(*n.a, v));
    case EXPR_FLOOR: return std::floor(direct(*n.a, v));
    case EXPR_SQRT: return std::sqrt(direct(*n.a, v));
    case EXPR_MOD: return std::fmod(direct(*n.a, v), direct(*n.b, v));
    default: return (double)((int64_t)direct(*n.a, v) / (int64_t)direct(*n.b, v));  // EXPR_LDIV: integers by construction
  }
}

int check_programs() {
  int accepted = 0, with_new = 0;
  for (int t = 0; t < 20000; ++t) {
    const auto tree = gen_num(1 + (int)(rnd() % 4));
    std::vector<ExprOpIn> ops;
    emit(*tree, &ops);
    ExprProg prog;
    const int rc = expr_compile(ops.data(), (int)ops.size(), &prog);
    if (rc == EXPR_BAD_LENGTH || rc == EXPR_TOO_DEEP || rc == EXPR_TOO_MANY_COLUMNS || rc == EXPR_NO_COLUMN) continue;
    if (rc != EXPR_OK) {
      ++g_bad;
      printf("MISMATCH a well-formed program is refused: %d %s\n", rc, expr_error_text(rc));
      continue;
    }
    ++accepted;
    bool any_new = false;
    for (const ExprOpIn& o : ops) any_new |= o.op >= EXPR_ABS;
    with_new += any_new;
    for (int r = 0; r < 8; r += 2) {
      double table[2][4], v[kExprMaxCols][2] = {}, out[2];
      for (int d = 0; d < 2; ++d) {
        const double specials[] = {0.0, -0.0, 0.5, -1.5, kInf, -kInf, kNaN, 2.25};
        table[d][0] = (double)((int64_t)(rnd() >> 34) - (1ll << 29));
        table[d][1] = (r + d) % 4 == 0 ? (double)((1ll << 30) - 1) * ((r + d) % 8 ? -1 : 1) : (double)((int64_t)(rnd() % 200001) - 100000);
        table[d][2] = (r + d) < 6 ? (double)(int64_t)(rnd() >> 11) / 4503599627370496.0 * 64.0 - 32.0 : specials[rnd() % 8];
        table[d][3] = (r + d) < 4 ? (double)(int64_t)(rnd() >> 40) : specials[rnd() % 8];
        for (int c = 0; c < prog.ncols; ++c) v[c][d] = table[d][prog.col[c]];
      }
      expr_eval<2>(prog, v, out);
      for (int d = 0; d < 2; ++d) {
        const double want = direct(*tree, table[d]);
        if (!same(out[d], want) || expr_value_key(out[d]) != expr_value_key(want)) {
          ++g_bad;
          printf("MISMATCH program %d row %d: got %.17g [%016" PRIx64 "], want %.17g [%016" PRIx64 "]\n", t, r + d, out[d],
                 bits(out[d]), want, bits(want));
        }
      }
    }
  }
  if (accepted < 2000 || with_new < 1000) {
    ++g_bad;
    printf("MISMATCH only %d programs accepted, %d with a new op\n", accepted, with_new);
  }
  return with_new;
}

}  // namespace

int main() {
  printf("ok edges %d\n", check_edges());
  printf("ok ldiv %d\n", check_ldiv());
  printf("ok programs %d\n", check_programs());
  if (g_bad) printf("FAILED %d\n", g_bad);
  return g_bad ? 1 : 0;
}
