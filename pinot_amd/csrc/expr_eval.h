// expr_eval.h -- arithmetic expressions inside aggregations (SUM(price * qty)): the postfix program of a table's
// virtual column, its validation, its evaluation in IEEE double and the order-preserving key of the result.  One
// header for the host (the C ABI's validation, tools/expr_check.cpp) and the device (the scan's expression instances,
// device.h): both evaluate the same text, so a value has the same bits wherever it is computed.
//
// Semantics (the reference's arithmetic transform functions, core/operator/transform/function/): every operand is a
// double -- a column's getDoubleValuesSV value or Double.parseDouble of a literal -- and every operation rounds on its
// own.  No fused multiply-add: the device uses __dadd_rn / __dmul_rn / __ddiv_rn, which the compiler never contracts,
// and the host code is compiled with contraction off (the pragma below, and -ffp-contract=off in the tool's build).
// The n-ary ADD / MULT of the reference are emitted by the callers as left-to-right chains that start with the folded
// literal (0.0 + literals for ADD, 1.0 * literals for MULT), so the program only has binary operations.
//
// Conditional expressions (CASE WHEN a > 1 THEN b ELSE c END: CaseTransformFunction, BinaryOperatorTransformFunction,
// And / OrOperatorTransformFunction): a stack entry is a number or a boolean, and expr_compile checks which.
//   EQ NE GT GE LT LE  pop b, then a (numbers), push the boolean Double.compare(a, b) <op> 0.  Double.compare is the
//                      total order of Double.doubleToLongBits -- -0.0 below +0.0, every NaN one value that equals itself
//                      and lies above +inf -- which is the signed order of expr_value_key: the keys are compared.  This
//                      is NOT the rule of the WHERE predicate evaluators (PredicateEvaluator), where 0.0 == -0.0.
//   AND OR             pop two booleans, push one (the reference's n-ary form is a left-to-right chain).
//   SELECT             pops cond (top, a boolean), then `then`, then `else` (numbers); pushes cond ? then : else.  CASE
//                      WHEN c1 THEN r1 .. WHEN cN THEN rN ELSE e END is e, rN, cN, SELECT, .., r1, c1, SELECT: the first
//                      matching WHEN wins (getSelectedArray).  Every branch is evaluated for every doc, only the selection
//                      differs: x / 0 in an unselected branch is harmless.
// A boolean is the double 1.0 or 0.0 in the same stack rows.  Since a boolean is only ever made above the two numbers
// its SELECT will read, a chain of two comparisons joined by AND / OR needs five entries, one more than the stack has:
// callers lower such conditions to further SELECTs (pinot_amd/query.py: expr_program), and AND / OR are accepted where
// they fit the type rules and refused by the depth limit like any other program that is too deep.
// The VM is all-double.  Bit parity with the reference therefore is the caller's duty for literals (include/pinotgpu.h,
// pgpu_expr_opcode): each literal is given as the double the reference reads under its type.
//
// Math and time functions (SingleParamMathTransformFunction, ModuloTransformFunction, TimeConversionTransformFunction,
// DateTimeConversionTransformFunction's epoch-to-epoch form):
//   ABS CEIL FLOOR SQRT  number -> number, the depth stays: Java's Math.abs / ceil / floor / sqrt, all correctly rounded
//                      (abs(-0.0) is +0.0, ceil(-0.5) is -0.0, sqrt of a negative is NaN, sqrt(-0.0) is -0.0).
//   MOD                pop b, then a; push a % b of Java's doubles, C's fmod: exact, the dividend's sign.
//   LDIV               pop b, then a; push (double)((long)a / (long)b): the truncating division of two longs held in
//                      doubles.  expr_compile admits it only where that reading is exact: b is the literal right before
//                      it, a positive integer of at most 2^53, and a is integral -- an INT / LONG column
//                      (expr_integral_columns: the caller checks the types), MULT of an integral value and a positive
//                      integer literal, or another LDIV.  Within +-2^53 (the plan checks every chain against the
//                      dictionaries: expr_chains_exact) the quotient of the doubles, truncated and put right by the exact
//                      remainder, is the quotient of the longs.  A zero quotient is +0.0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // __dadd_rn and its kin
#define PGPU_HD __host__ __device__
#else
#define PGPU_HD
#endif

namespace pgpu {

constexpr int kExprMaxOps = 16;    // ops of one program
constexpr int kExprMaxDepth = 4;   // values on the evaluation stack
constexpr int kExprMaxCols = 4;    // distinct columns of one program
constexpr int kMaxTableExprs = 256;  // expressions registered on one table
constexpr int kMaxPlanExprs = 8;   // distinct expressions aggregated by one plan

enum ExprOpCode : int32_t {
  EXPR_COLUMN = 0, EXPR_LITERAL = 1, EXPR_ADD = 2, EXPR_SUB = 3, EXPR_MULT = 4, EXPR_DIV = 5,
  EXPR_EQ = 6, EXPR_NE = 7, EXPR_GT = 8, EXPR_GE = 9, EXPR_LT = 10, EXPR_LE = 11, EXPR_AND = 12, EXPR_OR = 13,
  EXPR_SELECT = 14,
  // (15 is no op: the code the suite pins as the unknown one)
  EXPR_ABS = 16, EXPR_CEIL = 17, EXPR_FLOOR = 18, EXPR_SQRT = 19, EXPR_MOD = 20, EXPR_LDIV = 21
};
constexpr double kExprExact = 9007199254740992.0;  // 2^53: up to here every integer is a double

// One op as the caller states it (the layout of pgpu_expr_op, include/pinotgpu.h).
struct ExprOpIn {
  int32_t op;
  int32_t column;
  double literal;
};

// A validated program.  code[k] = op | arg << 8: EXPR_COLUMN's arg indexes col[] (the program's distinct columns in
// first-use order: table columns as registered, the plan's record indexes inside KParamsExpr), EXPR_LITERAL's indexes
// lit[].
struct ExprProg {
  int32_t nops;
  int32_t ncols;
  int32_t col[kExprMaxCols];
  int32_t code[kExprMaxOps];
  double lit[kExprMaxOps];
};

// The operand columns of a program in one segment as the device reads them, operand c being P.col[c]: the MSB-first
// fixed-bit forward index (padded), the dictId -> double table and the dictIds' width.  The first member of the tasks of
// both kernels that evaluate a program per doc (KExprLeafTask, internal.h; KDeriveTask, derive.h).
struct ExprOperands {
  const uint32_t* fwd[kExprMaxCols];
  const double* dval[kExprMaxCols];
  int32_t bits[kExprMaxCols];
};
// ... of program P in segment s (rt.h's Segment, whose d_val the caller has made: ensure_values; a template so that the
// host check of the leaves' tasks, which has no device runtime, fills its tasks here too).  Unused operands stay null.
template <typename Seg>
inline ExprOperands expr_operands(const Seg& s, const ExprProg& P) {
  ExprOperands o = {};
  for (int c = 0; c < P.ncols && c < kExprMaxCols; ++c) {
    const auto& col = s.cols[P.col[c]];
    o.fwd[c] = col.d_fwd;
    o.dval[c] = col.d_val;
    o.bits[c] = col.bits;
  }
  return o;
}

// The stack shape of an op: how many entries it reads -- 0 a push (COLUMN, LITERAL), 1 ABS .. SQRT, 2 the binary ops,
// 3 SELECT -- or -1 for a code that is no op (15 among them).  Every op leaves one entry, so the depth changes by
// 1 - pops.  The one table of the host's walkers (expr_compile, expr_compared_columns, expr_walk_chains, and the C ABI's
// default name); the device dispatches for itself (expr_stack_op).
constexpr int expr_op_pops(int op) {
  return op == EXPR_COLUMN || op == EXPR_LITERAL                               ? 0
         : op >= EXPR_ABS && op <= EXPR_SQRT                                   ? 1
         : (op >= EXPR_ADD && op <= EXPR_OR) || op == EXPR_MOD || op == EXPR_LDIV ? 2
         : op == EXPR_SELECT                                                   ? 3
                                                                               : -1;
}

enum ExprError : int {
  EXPR_OK = 0, EXPR_BAD_LENGTH, EXPR_BAD_OP, EXPR_UNDERFLOW, EXPR_TOO_DEEP, EXPR_TOO_MANY_COLUMNS, EXPR_LEFTOVER,
  EXPR_NO_COLUMN, EXPR_BAD_COLUMN, EXPR_BAD_TYPE, EXPR_BAD_DIVISOR, EXPR_BAD_DIVIDEND, EXPR_BAD_MATH_TYPE
};
inline const char* expr_error_text(int e) {
  switch (e) {
    case EXPR_OK: return "ok";
    case EXPR_BAD_LENGTH: return "a program has 1 to 16 ops";
    case EXPR_BAD_OP: return "unknown op";
    case EXPR_UNDERFLOW: return "stack underflow";
    case EXPR_TOO_DEEP: return "stack deeper than 4";
    case EXPR_TOO_MANY_COLUMNS: return "more than 4 distinct columns";
    case EXPR_LEFTOVER: return "the program does not leave exactly one value";
    case EXPR_NO_COLUMN: return "no column operand";
    case EXPR_BAD_TYPE:
      return "bad operand type: arithmetic and comparisons take numbers, AND / OR booleans, SELECT (number, number, "
             "boolean), and the program leaves a number";
    case EXPR_BAD_DIVISOR:
      return "LDIV's divisor is the LITERAL right before it, a positive integer of at most 2^53";
    case EXPR_BAD_DIVIDEND:
      return "LDIV's dividend is integral: an INT or LONG column, MULT of an integral value and a positive integer "
             "literal, or another LDIV";
    case EXPR_BAD_MATH_TYPE: return "bad operand type: ABS, CEIL, FLOOR, SQRT, MOD and LDIV take numbers, not booleans";
    default: return "negative column";
  }
}

// Validates ops[0, n) and compiles them into *out.  Column indexes are only required to be >= 0 here (the caller knows
// the table).  `boolean` has bit d set where stack entry d (0 = the bottom) is a boolean.
inline int expr_compile(const ExprOpIn* ops, int n, ExprProg* out) {
  *out = ExprProg{};
  if (!ops || n < 1 || n > kExprMaxOps) return EXPR_BAD_LENGTH;
  int depth = 0, nlit = 0;
  // `integral` likewise where entry d is an integral value (an LDIV's dividend; a column provisionally: its type is the
  // caller's to check, expr_integral_columns), `posint` where it is a positive integer literal of at most 2^53.
  uint32_t boolean = 0, integral = 0, posint = 0;
  auto bit = [&](uint32_t m, int from_top) { return (m >> (depth - 1 - from_top)) & 1u; };
  auto is_bool = [&](int from_top) { return bit(boolean, from_top); };
  for (int k = 0; k < n; ++k) {
    const int op = ops[k].op, pops = expr_op_pops(op);
    if (pops < 0) return EXPR_BAD_OP;
    if (depth < pops) return EXPR_UNDERFLOW;
    int arg = 0;
    bool r_bool = false, r_integral = false, r_posint = false;  // what the entry the op leaves is
    if (op == EXPR_COLUMN) {
      if (ops[k].column < 0) return EXPR_BAD_COLUMN;
      int c = 0;
      while (c < out->ncols && out->col[c] != ops[k].column) ++c;
      if (c == out->ncols) {
        if (out->ncols == kExprMaxCols) return EXPR_TOO_MANY_COLUMNS;
        out->col[out->ncols++] = ops[k].column;
      }
      arg = c;
      r_integral = true;
    } else if (op == EXPR_LITERAL) {
      const double l = ops[k].literal;
      out->lit[nlit] = l;
      arg = nlit++;
      r_posint = l >= 1.0 && l <= kExprExact && l == (double)(int64_t)l;
    } else if (op >= EXPR_ADD && op <= EXPR_LE) {  // (number, number) -> number, or -> boolean of a comparison
      if (is_bool(0) || is_bool(1)) return EXPR_BAD_TYPE;
      // x, LITERAL n, MULT over an integral x is the long product x * n (the literal on top, as LDIV's divisor stands);
      // LITERAL, x, MULT is arithmetic's double product, as the n-ary MULT of a caller starts.
      r_integral = op == EXPR_MULT && bit(integral, 1) && bit(posint, 0);
      r_bool = op >= EXPR_EQ;
    } else if (pops == 1) {  // ABS .. SQRT: number -> number
      if (is_bool(0)) return EXPR_BAD_MATH_TYPE;
    } else if (op == EXPR_MOD || op == EXPR_LDIV) {
      if (is_bool(0) || is_bool(1)) return EXPR_BAD_MATH_TYPE;
      if (op == EXPR_LDIV) {
        if (ops[k - 1].op != EXPR_LITERAL || !bit(posint, 0)) return EXPR_BAD_DIVISOR;
        if (!bit(integral, 1)) return EXPR_BAD_DIVIDEND;
      }
      r_integral = op == EXPR_LDIV;
    } else if (op == EXPR_AND || op == EXPR_OR) {
      if (!is_bool(0) || !is_bool(1)) return EXPR_BAD_TYPE;
      r_bool = true;
    } else {  // EXPR_SELECT
      if (!is_bool(0) || is_bool(1) || is_bool(2)) return EXPR_BAD_TYPE;
    }
    depth += 1 - pops;
    if (depth > kExprMaxDepth) return EXPR_TOO_DEEP;
    const uint32_t top = 1u << (depth - 1), below = top - 1u;
    boolean = (boolean & below) | (r_bool ? top : 0u);
    integral = (integral & below) | (r_integral ? top : 0u);
    posint = (posint & below) | (r_posint ? top : 0u);
    out->code[k] = op | (arg << 8);
  }
  if (depth != 1) return EXPR_LEFTOVER;
  if (boolean & 1u) return EXPR_BAD_TYPE;
  if (out->ncols == 0) return EXPR_NO_COLUMN;
  out->nops = n;
  return EXPR_OK;
}

PGPU_HD inline int64_t bits_of_double(double d) {
  int64_t b;
  __builtin_memcpy(&b, &d, 8);
  return b;
}

// Order-preserving int64 key of a double (the MIN / MAX operand): the bits of a positive value, the bits with their
// magnitude flipped of a negative one, so -0.0 (-1) sorts right below +0.0 (0).
PGPU_HD inline int64_t double_key_bits(double d) {
  const int64_t b = bits_of_double(d);
  return b >= 0 ? b : (b ^ INT64_MAX);
}
// ... of a computed value: every NaN is Double.doubleToLongBits's one (0x7ff8000000000000), as the NaN of a DOUBLE
// column is (rt_dict.cpp).
PGPU_HD inline int64_t expr_value_key(double d) {
  return d != d ? (int64_t)0x7ff8000000000000ll : double_key_bits(d);
}

// One operation, rounded on its own.
PGPU_HD inline double expr_apply(int op, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return op == EXPR_ADD ? __dadd_rn(a, b) : op == EXPR_SUB ? __dsub_rn(a, b) : op == EXPR_MULT ? __dmul_rn(a, b)
                                                                                               : __ddiv_rn(a, b);
#else
#pragma clang fp contract(off)
  return op == EXPR_ADD ? a + b : op == EXPR_SUB ? a - b : op == EXPR_MULT ? a * b : a / b;
#endif
}

// ABS / CEIL / FLOOR / SQRT: one instruction each on the device (v_and, v_ceil_f64, v_floor_f64) but the square root,
// which is the correctly rounded sequence of __dsqrt_rn.
PGPU_HD inline double expr_unary(int op, double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return op == EXPR_ABS ? __builtin_fabs(a) : op == EXPR_CEIL ? __builtin_ceil(a) : op == EXPR_FLOOR ? __builtin_floor(a)
                                                                                                     : __dsqrt_rn(a);
#else
  return op == EXPR_ABS ? __builtin_fabs(a) : op == EXPR_CEIL ? __builtin_ceil(a) : op == EXPR_FLOOR ? __builtin_floor(a)
                                                                                                     : __builtin_sqrt(a);
#endif
}

// (double)((long)a / (long)b) for integers |a| <= 2^53 and 1 <= b <= 2^53 held in doubles, without a 64-bit integer
// division.  a / b rounds to nearest, so its truncation is the quotient or, where the exact quotient lies just under an
// integer that it rounds up to, one further from zero.  The remainder a - q * b of either candidate is an integer of
// magnitude at most b <= 2^53, so the one rounding of a fused multiply-add returns it exactly, and its sign against a's
// tells which candidate q is.  Adding +0.0 turns a -0.0 quotient (-1 / 86400000) into +0.0, as a long has one zero.
PGPU_HD inline double expr_ldiv(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  double q = __builtin_trunc(__ddiv_rn(a, b));
#else
  double q = __builtin_trunc(a / b);
#endif
  const double r = __builtin_fma(-q, b, a);
  if (a >= 0.0 ? r < 0.0 : r > 0.0) q += a >= 0.0 ? -1.0 : 1.0;
  return q + 0.0;
}

// MOD and LDIV.  The device's fmod is the library's exact one (the compiler's own expansion of a remainder,
// x - trunc(x / y) * y, is not, so no builtin here).
PGPU_HD inline double expr_divide(int op, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return op == EXPR_MOD ? ::fmod(a, b) : expr_ldiv(a, b);
#else
  return op == EXPR_MOD ? __builtin_fmod(a, b) : expr_ldiv(a, b);
#endif
}

// The columns of P (a mask over P.col[]) whose value reaches a comparison as it is: pushed and compared, or passed on
// by SELECTs only.  The reference compares such an INT / LONG operand as an integer and this VM as a double, which is
// the same thing within +-2^53: the plan checks the dictionaries of these columns.
inline uint32_t expr_compared_columns(const ExprProg& P) {
  uint32_t st[kExprMaxDepth + 1] = {}, marked = 0;
  int depth = 0;
  for (int k = 0; k < P.nops; ++k) {
    const int op = P.code[k] & 0xFF, arg = P.code[k] >> 8, pops = expr_op_pops(op);
    if (pops < 0 || depth < pops) break;  // (no compiled program)
    uint32_t r = 0;  // the columns whose value the entry the op leaves is
    if (op == EXPR_COLUMN) r = 1u << arg;
    else if (op == EXPR_SELECT) r = st[depth - 3] | st[depth - 2];  // else | then (the condition is no value)
    else if (op >= EXPR_EQ && op <= EXPR_LE) marked |= st[depth - 1] | st[depth - 2];
    depth -= pops;
    st[depth++] = r;
  }
  return marked;
}

// The integral chains of P: a chain starts at a column and goes on through x, LITERAL n, MULT and x, LITERAL n, LDIV (n a
// positive integer of at most 2^53; what expr_compile calls integral), and ends where any other op reads it.  `visit`
// is called for every chain op as visit(chain, op, n) before chain.len, the count of chain ops so far, goes up; lo / hi /
// live are the visitor's to keep per chain.  A false answer ends the walk with false.
struct ExprChain {
  int col;  // of P.col[]; < 0: no chain value
  int len;
  int64_t lo, hi;
  bool live;
};
template <typename Visit>
inline bool expr_walk_chains(const ExprProg& P, Visit&& visit) {
  ExprChain st[kExprMaxDepth + 1] = {};
  int depth = 0;
  for (int k = 0; k < P.nops; ++k) {
    const int op = P.code[k] & 0xFF, arg = P.code[k] >> 8, pops = expr_op_pops(op);
    if (pops < 0 || depth < pops) break;  // (no compiled program)
    ExprChain r = {-1, 0, 0, 0, false};  // what the op leaves: no chain value, but for a column and a chain op
    if (op == EXPR_COLUMN) {
      r.col = arg;
    } else if (op == EXPR_MULT || op == EXPR_LDIV) {
      const int prev = k > 0 ? P.code[k - 1] : 0;
      const double n = (prev & 0xFF) == EXPR_LITERAL ? P.lit[prev >> 8] : 0.0;
      const bool posint = n >= 1.0 && n <= kExprExact && n == (double)(int64_t)n;
      ExprChain& e = st[depth - 2];
      if (posint && e.col >= 0) {
        if (!visit(e, op, (int64_t)n)) return false;
        ++e.len;
        r = e;
      }
    }
    depth -= pops;
    st[depth++] = r;
  }
  return true;
}

// The columns of P (a mask over P.col[]) that an LDIV divides, directly or through a chain: they are to be INT or LONG
// columns, which the caller -- who knows the table -- checks at registration.
inline uint32_t expr_integral_columns(const ExprProg& P) {
  uint32_t mask = 0;
  expr_walk_chains(P, [&](ExprChain& e, int op, int64_t) {
    if (op == EXPR_LDIV) mask |= 1u << e.col;
    return true;
  });
  return mask;
}

// Whether every integral chain of P stays within +-2^53 -- where a double is the long, and short of where Java's
// TimeUnit saturates -- at its column, at every intermediate value and at its result.  range(c, &lo, &hi) gives the
// least and greatest value of column c of P.col[] (a sorted dictionary's ends) and answers false for a column that
// holds no integers (FLOAT / DOUBLE: its chain is plain double arithmetic) or no values.  Every constant is positive,
// so a chain is monotone and its ends are those of its values; the arithmetic is exact (overflow is detected).
inline bool expr_within_exact(int64_t lo, int64_t hi) {  // the integers [lo, hi] are their doubles
  return lo >= -(int64_t)kExprExact && hi <= (int64_t)kExprExact;
}
template <typename Range>
inline bool expr_chains_exact(const ExprProg& P, Range&& range) {
  return expr_walk_chains(P, [&](ExprChain& e, int op, int64_t n) {
    if (e.len == 0) {
      e.live = range(e.col, &e.lo, &e.hi);
      if (e.live && !expr_within_exact(e.lo, e.hi)) return false;
    }
    if (!e.live) return true;
    if (op == EXPR_LDIV) {
      e.lo /= n;
      e.hi /= n;
    } else if (__builtin_mul_overflow(e.lo, n, &e.lo) || __builtin_mul_overflow(e.hi, n, &e.hi)) {
      return false;
    }
    return expr_within_exact(e.lo, e.hi);
  });
}

// A comparison's outcomes as a mask over (a < b, a == b, a > b) in the total order: bits 0, 1, 2.
PGPU_HD inline int expr_cmp_mask(int op) {
  return op == EXPR_EQ ? 2 : op == EXPR_NE ? 5 : op == EXPR_GT ? 4 : op == EXPR_GE ? 6 : op == EXPR_LT ? 1 : 3;
}

// A comparison in the total order, m = expr_cmp_mask(op): per lane, without a branch (v_cmp / v_cndmask).
PGPU_HD inline double expr_compare(int m, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  // The order of the keys without making them: the IEEE compares, which answer in lane masks, put right where the total
  // order differs -- -0.0 below +0.0, a NaN above everything and equal to a NaN (v_cmp_class: 0x3 the NaNs, 0x20 -0.0,
  // 0x40 +0.0).  No register is spent on a key.
  const bool a_nan = __builtin_amdgcn_class(a, 0x3), b_nan = __builtin_amdgcn_class(b, 0x3);
  const bool lt = a < b || (__builtin_amdgcn_class(a, 0x20) && __builtin_amdgcn_class(b, 0x40)) || (!a_nan && b_nan);
  const bool gt = a > b || (__builtin_amdgcn_class(a, 0x40) && __builtin_amdgcn_class(b, 0x20)) || (a_nan && !b_nan);
#else
  const int64_t ka = expr_value_key(a), kb = expr_value_key(b);
  const bool lt = ka < kb, gt = ka > kb;
#endif
  return ((lt && (m & 1)) || (!lt && !gt && (m & 2)) || (gt && (m & 4))) ? 1.0 : 0.0;
}

// AND / OR of two booleans (1.0 / 0.0): their minimum / maximum, one instruction on the doubles as they are.
PGPU_HD inline double expr_logic(int op, double a, double b) {
  return op == EXPR_AND ? __builtin_fmin(a, b) : __builtin_fmax(a, b);
}

// One stack operation other than a push on the four stack rows of N docs (s0 the top).  The op is the same for all
// lanes of a wave and is dispatched once, outside the docs' loops.
template <int N>
PGPU_HD inline void expr_stack_op(int op, double (&s0)[N], double (&s1)[N], double (&s2)[N], double (&s3)[N]) {
  if (__builtin_expect(op <= EXPR_DIV, 1)) {  // (arithmetic first and the rest laid out behind it)
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = expr_apply(op, s1[b], s0[b]);
      s1[b] = s2[b];
      s2[b] = s3[b];
    }
  } else if (op <= EXPR_LE) {
    const int m = expr_cmp_mask(op);
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = expr_compare(m, s1[b], s0[b]);
      s1[b] = s2[b];
      s2[b] = s3[b];
    }
  } else if (op == EXPR_SELECT) {  // (cond, then, else) -> one value: two entries leave
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = s0[b] != 0.0 ? s1[b] : s2[b];
      s1[b] = s3[b];
    }
  } else if (op < EXPR_SELECT) {
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = expr_logic(op, s1[b], s0[b]);
      s1[b] = s2[b];
      s2[b] = s3[b];
    }
  } else if (op < EXPR_SQRT) {  // (the math and time ops last: the programs without them fetch what they fetched)
#pragma unroll
    for (int b = 0; b < N; ++b) s0[b] = expr_unary(op, s0[b]);
  } else if (op == EXPR_SQRT) {  // (the long sequences each behind a branch of their own)
#pragma unroll
    for (int b = 0; b < N; ++b) s0[b] = expr_unary(EXPR_SQRT, s0[b]);
  } else if (op == EXPR_LDIV) {
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = expr_divide(EXPR_LDIV, s1[b], s0[b]);
      s1[b] = s2[b];
      s2[b] = s3[b];
    }
  } else {
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = expr_divide(EXPR_MOD, s1[b], s0[b]);
      s1[b] = s2[b];
      s2[b] = s3[b];
    }
  }
}

// Evaluates program P for NB docs at once: v[c][b] is column operand c (P.col[c]) of doc b, out[b] the result.  The
// stack is four named rows that shift (s0 is the top), so nothing is indexed by a run-time value and every row stays in
// registers; the program and its length are the same for all lanes of a wave.
template <int NB, typename Prog>
PGPU_HD inline void expr_eval(const Prog& P, const double (&v)[kExprMaxCols][NB], double (&out)[NB]) {
  double s0[NB], s1[NB], s2[NB], s3[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) s0[b] = s1[b] = s2[b] = s3[b] = 0.0;
  const int n = P.nops;
  for (int k = 0; k < n; ++k) {
    const int code = P.code[k], op = code & 0xFF, arg = code >> 8;
    if (op == EXPR_COLUMN || op == EXPR_LITERAL) {
      const double lit = op == EXPR_LITERAL ? P.lit[arg] : 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        s3[b] = s2[b];
        s2[b] = s1[b];
        s1[b] = s0[b];
        s0[b] = op == EXPR_LITERAL ? lit : arg == 0 ? v[0][b] : arg == 1 ? v[1][b] : arg == 2 ? v[2][b] : v[3][b];
      }
    } else {
      expr_stack_op<NB>(op, s0, s1, s2, s3);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) out[b] = s0[b];
}

}  // namespace pgpu
