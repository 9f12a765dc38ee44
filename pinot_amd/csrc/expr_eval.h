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

enum ExprOpCode : int32_t { EXPR_COLUMN = 0, EXPR_LITERAL = 1, EXPR_ADD = 2, EXPR_SUB = 3, EXPR_MULT = 4, EXPR_DIV = 5 };

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
  EXPR_NO_COLUMN, EXPR_BAD_COLUMN
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
    default: return "negative column";
  }
}

// Validates ops[0, n) and compiles them into *out.  Column indexes are only required to be >= 0 here (the caller knows
// the table).
inline int expr_compile(const ExprOpIn* ops, int n, ExprProg* out) {
  *out = ExprProg{};
  if (!ops || n < 1 || n > kExprMaxOps) return EXPR_BAD_LENGTH;
  int depth = 0, nlit = 0;
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
    } else if (op >= EXPR_ADD && op <= EXPR_DIV) {
      if (depth < 2) return EXPR_UNDERFLOW;
      --depth;
    } else {
      return EXPR_BAD_OP;
    }
    if (depth > kExprMaxDepth) return EXPR_TOO_DEEP;
    out->code[k] = op | (arg << 8);
  }
  if (depth != 1) return EXPR_LEFTOVER;
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
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        s0[b] = expr_apply(op, s1[b], s0[b]);
        s1[b] = s2[b];
        s2[b] = s3[b];
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) out[b] = s0[b];
}

}  // namespace pgpu
