// fx_agree_check.cpp -- host check of the cross-rank agreement on the fixed-point format of FLOAT / DOUBLE sums
// (pinot_amd/csrc/fx_sum.h: FxAgree, fx_agree_merge; nothing else of the library is included or linked).  Built under
// AddressSanitizer + UndefinedBehaviorSanitizer by pinot_amd.build.build_fx_agree_check, run by
// tests/test_fp_sum_agree_cpu.py.
//
// R synthetic ranks hold operands of different magnitudes (one rank the large ones, the others ever smaller ones, one
// rank none at all).  Every rank reports its range and docs, the reports are merged by fx_agree_merge, and every rank
// splits its operands in the one agreed format and sums the digits as int64 (any overflow is a failure); the ranks'
// digit sums are added -- forwards, backwards and pairwise, as an all-reduce, a ring or a tree would -- and converted
// once.  The result must equal a long-integer reference over the operands of all ranks (a 2240-bit fixed-point
// accumulator whose bit 0 is 2^-1074, rounded to nearest-even once), whatever the order of the ranks.
// Exit status 0 = all held.  --local-formats lets each rank split in the format of its own operands and docs (what
// plain plans do): the digit sums of unlike formats are added all the same, and the check must fail (the test asserts
// that it does) -- that is why the ranks agree first.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fx_sum.h"

using namespace pgpu;

static bool g_local = false;
static long long g_cases = 0, g_failures = 0, g_differing = 0;

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
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

static void ref_add(Big* pos, Big* neg, double v, bool quantised, int quantum) {
  if (v == 0.0) return;
  int e;
  const double m = frexp(fabs(v), &e);
  uint64_t mant = (uint64_t)ldexp(m, 53);
  e -= 53;
  if (e < -1074) { mant >>= -1074 - e; e = -1074; }
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

static double rnd_value(int emin, int emax, int mant_bits) {
  const uint64_t mant = (rnd() >> (64 - mant_bits)) | 1ull;  // odd: the lowest bit is set
  const int e = emin + (int)(rnd() % (uint64_t)(emax - emin + 1));
  const double v = ldexp((double)mant, e - mant_bits);
  return (rnd() & 1) ? -v : v;
}

static FxRange range_of(const FxAgree& a) {
  FxRange r;
  r.E = a.E;
  r.L = a.L;
  r.any = a.any != 0;
  r.finite = a.finite != 0;
  return r;
}

static bool same_format(const FxFormat& a, const FxFormat& b) {
  return a.mode == b.mode && a.E == b.E && a.K == b.K && a.W == b.W;
}

struct Sums {
  int64_t d[kFxMaxDigits] = {0, 0, 0};
};

static bool add_sums(Sums* a, const Sums& b) {
  bool overflow = false;
  for (int j = 0; j < kFxMaxDigits; ++j) overflow |= __builtin_add_overflow(a->d[j], b.d[j], &a->d[j]);
  return overflow;
}

static void fail_case(const char* name, const char* what) {
  if (++g_failures <= 20) printf("FAIL %s: %s\n", name, what);
}

// ranks[r]: the operands of rank r
static void run_case(const char* name, const std::vector<std::vector<double>>& ranks) {
  ++g_cases;
  const int R = (int)ranks.size();
  std::vector<FxAgree> mine(R);
  for (int r = 0; r < R; ++r) {
    FxRange rg;
    for (double x : ranks[r]) fx_range_add(&rg, x);
    FxAgree& a = mine[r];
    a.is_sum = 1;
    a.any = rg.any;
    a.finite = rg.finite;
    a.E = rg.any ? rg.E : 0;
    a.L = rg.any ? rg.L : 0;
    a.docs = (int64_t)ranks[r].size();
  }
  FxAgree agreed;
  if (fx_agree_merge(mine.data(), R, 1, &agreed)) return fail_case(name, "the merge refused ranks of one aggregation");
  // the merge does not depend on the order of the ranks
  {
    std::vector<FxAgree> rev(mine.rbegin(), mine.rend());
    FxAgree other;
    if (fx_agree_merge(rev.data(), R, 1, &other) || memcmp(&other, &agreed, sizeof agreed))
      return fail_case(name, "the merged range depends on the order of the ranks");
  }
  int64_t docs = 0;
  for (const auto& v : ranks) docs += (int64_t)v.size();
  if (agreed.docs != docs) return fail_case(name, "the agreed docs are not the sum of the ranks' docs");
  const FxFormat f = fx_format(range_of(agreed), agreed.docs);
  if (f.mode == FX_NONE || f.W < 2 || f.W > kFxMaxDigits) return fail_case(name, "no format");
  bool differs = false;
  std::vector<Sums> part(R);
  for (int r = 0; r < R; ++r) {
    const FxFormat own = fx_format(range_of(mine[r]), mine[r].docs);
    differs |= !same_format(own, f);
    const FxFormat& use = g_local ? own : f;
    for (double x : ranks[r])
      for (int j = 0; j < use.W; ++j) {
        const double d = fx_digit_f64(x, use.K - use.E, use.K, j);
        if (!(fabs(d) < ldexp(1.0, use.K))) return fail_case(name, "a digit is not below 2^K");
        if (__builtin_add_overflow(part[r].d[j], (int64_t)d, &part[r].d[j])) return fail_case(name, "int64 overflow of a rank's digit sum");
      }
  }
  g_differing += differs;
  // the ranks' digit sums added forwards, backwards and pairwise (a tree): integer sums, so one answer
  Sums fwd, bwd;
  bool overflow = false;
  for (int r = 0; r < R; ++r) overflow |= add_sums(&fwd, part[r]);
  for (int r = R - 1; r >= 0; --r) overflow |= add_sums(&bwd, part[r]);
  std::vector<Sums> tree(part);
  for (int step = 1; step < R; step *= 2)
    for (int r = 0; r + step < R; r += 2 * step) overflow |= add_sums(&tree[r], tree[r + step]);
  if (overflow) return fail_case(name, "int64 overflow of a merged digit sum");
  if (memcmp(&fwd, &bwd, sizeof fwd) || memcmp(&fwd, &tree[0], sizeof fwd)) return fail_case(name, "the merged digit sums depend on the merge order");
  if (!(llabs(fwd.d[0]) < (INT64_C(1) << 61))) return fail_case(name, "a merged digit sum passes 2^61");
  const double got = fx_result(fwd.d, f);
  Big pos, neg;
  for (const auto& v : ranks)
    for (double x : v) ref_add(&pos, &neg, x, f.mode == FX_QUANTISED, f.E - f.W * f.K);
  double want;
  if (pos.cmp(neg) >= 0) { pos.sub(neg); want = pos.to_double(); }
  else { neg.sub(pos); want = -neg.to_double(); }
  if (bits_of(got) != bits_of(want)) {
    if (++g_failures <= 20)
      printf("FAIL %s: %a, reference %a (ranks=%d docs=%lld mode=%d E=%d K=%d W=%d)\n", name, got, want, R,
             (long long)docs, f.mode, f.E, f.K, f.W);
  }
}

// The merge rule itself on hand-made reports: is_sum mismatches, non-finite ranks, ranks without operands, bounds.
static void check_rule() {
  ++g_cases;
  FxAgree a[3], out[1];
  a[0].is_sum = 1; a[0].any = 1; a[0].finite = 1; a[0].E = 55; a[0].L = 2; a[0].docs = 100; a[0].int_sum_bound = 0x1p61;
  a[1].is_sum = 1; a[1].any = 0; a[1].finite = 1; a[1].E = 0; a[1].L = 0; a[1].docs = 7; a[1].int_sum_bound = 0;
  a[2].is_sum = 1; a[2].any = 1; a[2].finite = 0; a[2].E = -3; a[2].L = -30; a[2].docs = 1; a[2].int_sum_bound = 0x1p61;
  if (fx_agree_merge(a, 3, 1, out) || !out[0].is_sum || !out[0].any || out[0].finite || out[0].E != 55 || out[0].L != -30 ||
      out[0].docs != 108 || out[0].int_sum_bound != 0x1p62)
    fail_case("rule", "three ranks (one without operands, one not finite)");
  if (fx_agree_merge(a, 2, 1, out) || !out[0].finite || out[0].E != 55 || out[0].L != 2 || out[0].docs != 107)
    fail_case("rule", "a rank without operands changed E or L");
  a[1].is_sum = 0;
  if (fx_agree_merge(a, 2, 1, out) != -1) fail_case("rule", "ranks that differ on is_sum were merged");
  FxAgree z[2];
  if (fx_agree_merge(z, 2, 1, out) || out[0].is_sum || out[0].docs || out[0].any) fail_case("rule", "a COUNT / MIN / MAX entry is not all zero");
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--local-formats")) g_local = true;
    else { printf("usage: fx_agree_check [--local-formats]\n"); return 2; }
  }
  check_rule();
  char name[96];
  std::vector<std::vector<double>> ranks;
  // rank 0 the large operands, the others ever smaller ones; one rank without any where R >= 3
  for (int c = 0; c < 120; ++c) {
    const int R = 1 + c % 8;
    ranks.assign(R, {});
    for (int r = 0; r < R; ++r) {
      if (R >= 3 && r == R - 1 && c % 2) continue;  // a rank whose segments hold no docs
      const size_t n = 1 + (size_t)(rnd() % (c < 40 ? 200 : 20000));
      const int hi = 55 - 9 * r, lo = hi - 12;
      for (size_t i = 0; i < n; ++i) ranks[r].push_back(rnd_value(lo, hi, c % 3 == 0 ? 24 : 10));
      if (c % 5 == 4) ranks[r].push_back(0.0);
    }
    snprintf(name, sizeof name, "magnitudes by rank %d (%d ranks)", c, R);
    run_case(name, ranks);
  }
  // the GPU test's data: one rank odd multiples of 4 near +-2^54, the other odd multiples of 2^-30
  for (int c = 0; c < 10; ++c) {
    ranks.assign(2, {});
    const size_t n = 2 + (size_t)(rnd() % 70000);
    for (size_t i = 0; i < n; ++i) {
      const double big = ldexp(1.0, 54) + 4.0 * (double)(2 * (rnd() % 1000) + 1);
      ranks[0].push_back(i & 1 ? big : -big);
      ranks[1].push_back(ldexp((double)(2 * (rnd() % 100000) + 1), -30));
    }
    snprintf(name, sizeof name, "large and small rank %d", c);
    run_case(name, ranks);
  }
  // wide: W = 3 exact and quantised agreed formats
  for (int c = 0; c < 20; ++c) {
    const int R = 2 + c % 4;
    ranks.assign(R, {});
    for (int r = 0; r < R; ++r) {
      const size_t n = 1 + (size_t)(rnd() % 3000);
      for (size_t i = 0; i < n; ++i)
        ranks[r].push_back(c & 1 ? rnd_value(40 - 50 * r, 60 - 50 * r, 53) : rnd_value(-20 - 20 * r, 10 - 20 * r, 53));
    }
    snprintf(name, sizeof name, "wide %d", c);
    run_case(name, ranks);
  }
  // the same operands dealt to the ranks another way: the same bits (run_case compares with the one reference)
  {
    std::vector<double> all;
    for (int i = 0; i < 30000; ++i) all.push_back(i % 3 ? rnd_value(40, 55, 20) : rnd_value(-30, -10, 20));
    for (int R = 1; R <= 8; ++R) {
      ranks.assign(R, {});
      for (size_t i = 0; i < all.size(); ++i) ranks[(i * 7 + i / 1000) % R].push_back(all[i]);
      snprintf(name, sizeof name, "one data set over %d ranks", R);
      run_case(name, ranks);
    }
  }
  if (!g_differing) {
    printf("FAIL no case had a rank whose own format differs from the agreed one\n");
    ++g_failures;
  }
  printf("%lld cases (%lld with a rank whose own format differs), %lld failures%s\n", g_cases, g_differing, g_failures,
         g_local ? " [each rank in its own format]" : "");
  return g_failures ? 1 : 0;
}
