// fx_sum_check.cpp -- host check of the fixed-point FLOAT / DOUBLE sum (pinot_amd/csrc/fx_sum.h, the header the
// kernels, the plan and the result conversion share; nothing else of the library is included or linked).  Built under
// AddressSanitizer + UndefinedBehaviorSanitizer by pinot_amd.build.build_fx_sum_check, run by
// tests/test_fx_sum_cpu.py.
//
// For sets of operands: format from their range, split of every operand, int64 digit sums (any overflow is a failure),
// conversion -- against a long-integer reference: every operand (truncated to the format's quantum when the format is
// quantised) added into a 2240-bit fixed-point accumulator whose bit 0 is 2^-1074, rounded to nearest-even once.
//   random      magnitudes 2^-30 .. 2^55 and wider, mixed signs, 1 .. 70 001 operands;
//   adversarial subnormals, +-DBL_MAX / 4, a single value, all zeros, alternating signs that cancel to 0;
//   formats     W = 2 exact, W = 3 exact and W = 3 quantised must each be met;
//   overflow    N up to 2^31 operands of the worst-case digits 2^K - 1 stay inside an int64.
// Exit status 0 = all held.  --no-headroom computes the formats with no headroom bits (K = 62): the digit sums
// overflow and the check must fail (the test asserts that it does).
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fx_sum.h"

using namespace pgpu;

static int g_headroom = -1;
static long long g_cases = 0, g_failures = 0;
static long long g_seen[3][4] = {};  // [mode][W]

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- the reference: unsigned magnitudes of the positive and the negative operands, bit 0 = 2^-1074
constexpr int kLimbs = 35;
struct Big {
  uint64_t w[kLimbs] = {};
  void add(uint64_t mant, int pos) {  // += mant 2^pos
    const int limb = pos >> 6, bit = pos & 63;
    unsigned __int128 x = (unsigned __int128)mant << bit;
    unsigned __int128 carry = 0;
    for (int i = limb; i < kLimbs; ++i) {
      carry += (unsigned __int128)w[i] + (uint64_t)x;
      x >>= 64;
      w[i] = (uint64_t)carry;
      carry >>= 64;
      if (!carry && !x) break;
    }
  }
  int cmp(const Big& o) const {
    for (int i = kLimbs - 1; i >= 0; --i)
      if (w[i] != o.w[i]) return w[i] < o.w[i] ? -1 : 1;
    return 0;
  }
  void sub(const Big& o) {  // this >= o
    uint64_t borrow = 0;
    for (int i = 0; i < kLimbs; ++i) {
      const unsigned __int128 d = (unsigned __int128)w[i] - o.w[i] - borrow;
      w[i] = (uint64_t)d;
      borrow = (uint64_t)(d >> 64) & 1u;
    }
  }
  uint64_t bit(int b) const { return b < 0 ? 0 : (w[b >> 6] >> (b & 63)) & 1u; }
  double to_double() const {
    int top = -1;
    for (int i = kLimbs - 1; i >= 0 && top < 0; --i)
      if (w[i]) top = 64 * i + 63 - __builtin_clzll(w[i]);
    if (top < 0) return 0.0;
    const int low = top - 52 > 0 ? top - 52 : 0;
    uint64_t mant = 0;
    for (int b = top; b >= low; --b) mant = (mant << 1) | bit(b);
    bool sticky = false;
    for (int b = low - 2; b >= 0 && !sticky; --b) sticky = bit(b) != 0;
    if (bit(low - 1) && (sticky || (mant & 1u))) ++mant;
    return ldexp((double)mant, low - 1074);
  }
};

// v = +-mant 2^e with mant < 2^53; quantum: bits below 2^quantum are cut off (truncation toward zero)
static void ref_add(Big* pos, Big* neg, double v, bool quantised, int quantum) {
  if (v == 0.0) return;
  int e;
  const double m = frexp(fabs(v), &e);
  uint64_t mant = (uint64_t)ldexp(m, 53);
  e -= 53;
  if (e < -1074) { mant >>= -1074 - e; e = -1074; }  // subnormals: the low bits are zero
  if (quantised && e < quantum) {
    const int s = quantum - e;
    mant = s >= 64 ? 0 : mant >> s;
    e = quantum;
  }
  if (mant) (v < 0 ? neg : pos)->add(mant, e + 1074);
}

static uint64_t bits_of(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}

static bool run_case(const char* name, const std::vector<double>& v) {
  ++g_cases;
  FxRange r;
  for (double x : v) fx_range_add(&r, x);
  const FxFormat f = fx_format(r, (int64_t)v.size(), g_headroom);
  if (f.mode == FX_NONE || f.W < 2 || f.W > kFxMaxDigits) {
    printf("FAIL %s: no format\n", name);
    ++g_failures;
    return false;
  }
  ++g_seen[f.mode][f.W];
  int64_t sums[kFxMaxDigits] = {0, 0, 0};
  bool overflow = false;
  for (double x : v)
    for (int j = 0; j < f.W; ++j) {
      const double d = fx_digit_f64(x, f.K - f.E, f.K, j);
      if (!(fabs(d) < ldexp(1.0, f.K))) {
        printf("FAIL %s: digit %d of %a is %a, not below 2^%d\n", name, j, x, d, f.K);
        ++g_failures;
        return false;
      }
      overflow |= __builtin_add_overflow(sums[j], (int64_t)d, &sums[j]);
    }
  if (overflow) {
    if (++g_failures <= 20)
      printf("FAIL %s: int64 overflow of a digit sum (n=%zu E=%d K=%d W=%d)\n", name, v.size(), f.E, f.K, f.W);
    return false;
  }
  const double got = fx_result(sums, f);
  Big pos, neg;
  for (double x : v) ref_add(&pos, &neg, x, f.mode == FX_QUANTISED, f.E - f.W * f.K);
  double want;
  if (pos.cmp(neg) >= 0) { pos.sub(neg); want = pos.to_double(); }
  else { neg.sub(pos); want = -neg.to_double(); }
  if (bits_of(got) != bits_of(want)) {
    if (++g_failures <= 20)
      printf("FAIL %s: %a, reference %a (n=%zu mode=%d E=%d K=%d W=%d)\n", name, got, want, v.size(), f.mode, f.E,
             f.K, f.W);
    return false;
  }
  return true;
}

static double rnd_value(int emin, int emax, int mant_bits) {
  const uint64_t mant = (rnd() >> (64 - mant_bits)) | 1ull;  // odd: the lowest bit is set
  const int e = emin + (int)(rnd() % (uint64_t)(emax - emin + 1));
  const double v = ldexp((double)mant, e - mant_bits);
  return (rnd() & 1) ? -v : v;
}

// N operands of the worst-case digit 2^K - 1 (both signs): N (2^K - 1) must stay inside an int64.
static void check_worst_case(int64_t n) {
  ++g_cases;
  const int H = g_headroom >= 0 ? g_headroom : fx_bit_length(n) + 1;
  const int K = 62 - H;
  const int64_t digit = (int64_t)((1ull << K) - 1);
  int64_t total;
  if (__builtin_mul_overflow(n, digit, &total) || __builtin_mul_overflow(n, -digit, &total)) {
    ++g_failures;
    printf("FAIL worst case: %lld digits of 2^%d - 1 overflow an int64\n", (long long)n, K);
    return;
  }
  if (g_headroom < 0 && !(total > -(INT64_C(1) << 61))) {
    ++g_failures;
    printf("FAIL worst case: %lld digits of 2^%d - 1 pass 2^61\n", (long long)n, K);
  }
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--no-headroom")) g_headroom = 0;
    else { printf("usage: fx_sum_check [--no-headroom]\n"); return 2; }
  }
  std::vector<double> v;
  char name[96];
  // random: 1 .. 70 001 operands, magnitudes 2^-30 .. 2^55, mixed signs; narrow mantissas keep W = 2 exact
  for (int c = 0; c < 200; ++c) {
    const size_t n = c < 8 ? (size_t)(c + 1) : 1 + (size_t)(rnd() % 70001);
    const int mant_bits = c % 3 == 0 ? 53 : c % 3 == 1 ? 20 : 3;
    v.clear();
    for (size_t i = 0; i < n; ++i) v.push_back(rnd_value(-30, 55, mant_bits));
    snprintf(name, sizeof name, "random %d (%d-bit mantissas)", c, mant_bits);
    run_case(name, v);
  }
  // wider: 2^-80 .. 2^60 (quantised at W = 3), and the whole double range
  for (int c = 0; c < 40; ++c) {
    const size_t n = 1 + (size_t)(rnd() % 5000);
    v.clear();
    for (size_t i = 0; i < n; ++i) v.push_back(c & 1 ? rnd_value(-80, 60, 53) : rnd_value(-1070, 1020, 53));
    snprintf(name, sizeof name, "wide %d", c);
    run_case(name, v);
  }
  // the GPU test's data: odd multiples of 4 near +-2^54 against odd multiples of 2^-30, partial cancellation
  for (int c = 0; c < 10; ++c) {
    const size_t n = 2 + (size_t)(rnd() % 70000);
    v.clear();
    for (size_t i = 0; i < n; ++i) {
      const double big = ldexp(1.0, 54) + 4.0 * (double)(2 * (rnd() % 1000) + 1);
      const double small = ldexp((double)(2 * (rnd() % 100000) + 1), -30);
      v.push_back(i % 3 == 0 ? big : i % 3 == 1 ? -big : small);
    }
    snprintf(name, sizeof name, "cancellation %d", c);
    run_case(name, v);
  }
  // subnormals
  v.clear();
  for (int i = 0; i < 5000; ++i) v.push_back(((rnd() & 1) ? -1.0 : 1.0) * ldexp((double)(1 + rnd() % 4096), -1074));
  run_case("subnormals", v);
  v.push_back(DBL_MIN);
  v.push_back(-ldexp(1.0, -1000));
  run_case("subnormals and small normals", v);
  // +-DBL_MAX / 4
  v = {DBL_MAX / 4, DBL_MAX / 4, -DBL_MAX / 4, DBL_MAX / 4, 1.0, -0.5, ldexp(1.0, -1074)};
  run_case("DBL_MAX / 4", v);
  v = {-DBL_MAX / 4, -DBL_MAX / 4, -DBL_MAX / 4};
  run_case("-DBL_MAX / 4", v);
  // a single value, all zeros, cancellation to 0
  for (double x : {1.0, -1.0, 0.1, -3.5e300, 4.9e-324, DBL_MAX, 1e-310, 12345.678}) {
    v = {x};
    run_case("single value", v);
  }
  v.assign(1000, 0.0);
  v[17] = -0.0;
  run_case("all zeros", v);
  v.clear();
  for (int i = 0; i < 4096; ++i) {
    const double x = rnd_value(-40, 40, 53);
    v.push_back(x);
    v.push_back(-x);
  }
  run_case("alternating signs that cancel", v);
  // rounding: ties and near-ties of the one final rounding
  v = {ldexp(1.0, 53), 1.0};
  run_case("tie to even (down)", v);
  v = {ldexp(1.0, 53) + 2.0, 1.0};
  run_case("tie to even (up)", v);
  v = {ldexp(1.0, 53), 1.0, ldexp(1.0, -20)};
  run_case("just above a tie", v);
  v = {-ldexp(1.0, 53), -1.0, ldexp(1.0, -20)};
  run_case("just below a tie, negative", v);
  // the worst-case digits: N up to 2^31
  for (int b = 0; b <= 31; ++b)
    for (int64_t d = -1; d <= 1; ++d) {
      const int64_t n = (INT64_C(1) << b) + d;
      if (n >= 1 && n <= (INT64_C(1) << 31)) check_worst_case(n);
    }
  // ... and summed for real at the largest sizes that take a moment: operands just below 2^E in every digit
  for (size_t n : {(size_t)3, (size_t)1000, (size_t)70001, (size_t)(1u << 20)}) {
    v.assign(n, nextafter(ldexp(1.0, 40), 0.0));
    run_case("all operands just below 2^E", v);
    for (size_t i = 0; i < n; i += 2) v[i] = -v[i];
    run_case("alternating operands just below 2^E", v);
  }
  if (g_headroom < 0) {
    const struct { int mode, W; const char* what; } need[] = {{FX_EXACT, 2, "W = 2 exact"}, {FX_EXACT, 3, "W = 3 exact"},
                                                              {FX_QUANTISED, 3, "W = 3 quantised"}};
    for (const auto& n : need)
      if (!g_seen[n.mode][n.W]) {
        printf("FAIL no case had a %s format\n", n.what);
        ++g_failures;
      }
  }
  printf("%lld cases (W=2 exact %lld, W=3 exact %lld, W=3 quantised %lld), %lld failures\n", g_cases,
         g_seen[FX_EXACT][2], g_seen[FX_EXACT][3], g_seen[FX_QUANTISED][3], g_failures);
  return g_failures ? 1 : 0;
}
