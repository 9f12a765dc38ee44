// case_check.cpp -- host check of conditional expression programs (pinot_amd/csrc/expr_eval.h: the comparisons, AND /
// OR, SELECT and the type check of expr_compile; nothing else of the library is included or linked).  Built under
// AddressSanitizer + UndefinedBehaviorSanitizer with floating-point contraction off by
// pinot_amd.build.build_case_check, run by tests/test_case_expr_cpu.py, which compares the printed bits with its own
// typed evaluation (tests/case_common.py).
//
// Input (stdin), a sequence of blocks:
//   prog N                      then N lines "c <column>" | "l <literal bits, hex>" | "o <opcode, decimal>"
//   rows R                      then R lines of the program's distinct columns' values (hex bits, in first-use order)
//   stack <opcode> <s0> <s1> <s2> <s3>      one stack operation (expr_stack_op) on the four rows, hex bits, s0 the top
// Output: for a program "error <code> <text>" where it does not validate (it has no rows then), else
// "ok <ncols> <compared columns, a mask>" and per row "<result bits, hex> <key, decimal>"; for a stack line the four
// rows afterwards.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "expr_eval.h"

namespace {

double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}

}  // namespace

int main() {
  char word[16];
  int n = 0;
  while (scanf("%15s %d", word, &n) == 2) {
    if (strcmp(word, "stack") == 0) {
      uint64_t b[4];
      if (scanf("%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &b[0], &b[1], &b[2], &b[3]) != 4) return 2;
      if (n < pgpu::EXPR_ADD || n > pgpu::EXPR_SELECT) return 2;
      double s[4][1] = {{from_bits(b[0])}, {from_bits(b[1])}, {from_bits(b[2])}, {from_bits(b[3])}};
      pgpu::expr_stack_op<1>(n, s[0], s[1], s[2], s[3]);
      printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", (uint64_t)pgpu::bits_of_double(s[0][0]),
             (uint64_t)pgpu::bits_of_double(s[1][0]), (uint64_t)pgpu::bits_of_double(s[2][0]),
             (uint64_t)pgpu::bits_of_double(s[3][0]));
      continue;
    }
    if (strcmp(word, "prog") != 0 || n < 0 || n > 1000) {
      fprintf(stderr, "expected `prog N` or `stack OP ...`\n");
      return 2;
    }
    std::vector<pgpu::ExprOpIn> ops((size_t)n);
    for (int k = 0; k < n; ++k) {
      char c[4];
      if (scanf("%3s", c) != 1) return 2;
      pgpu::ExprOpIn& o = ops[(size_t)k];
      o = pgpu::ExprOpIn{};
      if (c[0] == 'c') {
        o.op = pgpu::EXPR_COLUMN;
        if (scanf("%d", &o.column) != 1) return 2;
      } else if (c[0] == 'l') {
        uint64_t b = 0;
        o.op = pgpu::EXPR_LITERAL;
        if (scanf("%" SCNx64, &b) != 1) return 2;
        o.literal = from_bits(b);
      } else {
        if (scanf("%d", &o.op) != 1) return 2;
      }
    }
    int rows = 0;
    if (scanf("%15s %d", word, &rows) != 2 || strcmp(word, "rows") != 0 || rows < 0) {
      fprintf(stderr, "expected `rows R`\n");
      return 2;
    }
    pgpu::ExprProg prog;
    const int rc = pgpu::expr_compile(ops.data(), n, &prog);
    if (rc) {
      printf("error %d %s\n", rc, pgpu::expr_error_text(rc));
      if (rows) {
        fprintf(stderr, "rows after a program that does not validate\n");
        return 2;
      }
      continue;
    }
    printf("ok %d %u\n", prog.ncols, pgpu::expr_compared_columns(prog));
    for (int r = 0; r < rows; ++r) {
      double v[pgpu::kExprMaxCols][1] = {};
      for (int c = 0; c < prog.ncols; ++c) {
        uint64_t b = 0;
        if (scanf("%" SCNx64, &b) != 1) return 2;
        v[c][0] = from_bits(b);
      }
      double out[1];
      pgpu::expr_eval<1>(prog, v, out);
      printf("%016" PRIx64 " %" PRId64 "\n", (uint64_t)pgpu::bits_of_double(out[0]), pgpu::expr_value_key(out[0]));
    }
  }
  return 0;
}
