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
  EXPR_SELECT = 14
};

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

enum ExprError : int {
  EXPR_OK = 0, EXPR_BAD_LENGTH, EXPR_BAD_OP, EXPR_UNDERFLOW, EXPR_TOO_DEEP, EXPR_TOO_MANY_COLUMNS, EXPR_LEFTOVER,
  EXPR_NO_COLUMN, EXPR_BAD_COLUMN, EXPR_BAD_TYPE
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
    default: return "negative column";
  }
}

// Validates ops[0, n) and compiles them into *out.  Column indexes are only required to be >= 0 here (the caller knows
// the table).  `boolean` has bit d set where stack entry d (0 = the bottom) is a boolean.
inline int expr_compile(const ExprOpIn* ops, int n, ExprProg* out) {
  *out = ExprProg{};
  if (!ops || n < 1 || n > kExprMaxOps) return EXPR_BAD_LENGTH;
  int depth = 0, nlit = 0;
  uint32_t boolean = 0;
  auto is_bool = [&](int from_top) { return (boolean >> (depth - 1 - from_top)) & 1u; };
  for (int k = 0; k < n; ++k) {
    const int op = ops[k].op;
    int arg = 0;
    if (op == EXPR_COLUMN) {
      if (ops[k].column < 0) return EXPR_BAD_COLUMN;
      int c = 0;
      while (c < out->ncols && out->col[c] != ops[k].column) ++c;
      if (c == out->ncols) {
        if (out->ncols == kExprMaxCols) return EXPR_TOO_MANY_COLUMNS;
        out->col[out->ncols++] = ops[k].column;
      }
      arg = c;
      ++depth;
    } else if (op == EXPR_LITERAL) {
      out->lit[nlit] = ops[k].literal;
      arg = nlit++;
      ++depth;
    } else if (op >= EXPR_ADD && op <= EXPR_LE) {  // (number, number) -> number, or -> boolean of a comparison
      if (depth < 2) return EXPR_UNDERFLOW;
      if (is_bool(0) || is_bool(1)) return EXPR_BAD_TYPE;
      --depth;
      if (op >= EXPR_EQ) boolean |= 1u << (depth - 1);
    } else if (op == EXPR_AND || op == EXPR_OR) {
      if (depth < 2) return EXPR_UNDERFLOW;
      if (!is_bool(0) || !is_bool(1)) return EXPR_BAD_TYPE;
      --depth;
    } else if (op == EXPR_SELECT) {
      if (depth < 3) return EXPR_UNDERFLOW;
      if (!is_bool(0) || is_bool(1) || is_bool(2)) return EXPR_BAD_TYPE;
      depth -= 2;
    } else {
      return EXPR_BAD_OP;
    }
    if (depth > kExprMaxDepth) return EXPR_TOO_DEEP;
    boolean &= (1u << depth) - 1u;
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

// The columns of P (a mask over P.col[]) whose value reaches a comparison as it is: pushed and compared, or passed on
// by SELECTs only.  The reference compares such an INT / LONG operand as an integer and this VM as a double, which is
// the same thing within +-2^53: the plan checks the dictionaries of these columns.
inline uint32_t expr_compared_columns(const ExprProg& P) {
  uint32_t st[kExprMaxDepth + 1] = {}, marked = 0;
  int depth = 0;
  for (int k = 0; k < P.nops; ++k) {
    const int op = P.code[k] & 0xFF, arg = P.code[k] >> 8;
    if (op == EXPR_COLUMN) st[depth++] = 1u << arg;
    else if (op == EXPR_LITERAL) st[depth++] = 0;
    else if (op == EXPR_SELECT) { depth -= 2; st[depth - 1] |= st[depth]; }  // else | then (the condition is no value)
    else {
      if (op >= EXPR_EQ && op <= EXPR_LE) marked |= st[depth - 1] | st[depth - 2];
      --depth;
      st[depth - 1] = 0;
    }
  }
  return marked;
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
  } else {
#pragma unroll
    for (int b = 0; b < N; ++b) {
      s0[b] = expr_logic(op, s1[b], s0[b]);
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
