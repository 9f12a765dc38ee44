// fx_sum.h — order-independent FLOAT / DOUBLE sums (query option PGPU_OPT_EXACT_FP_SUM): every operand is split into
// W fixed-point digits of K bits, the digits are summed as int64 (exact, so in any order), and the W sums are put
// together and rounded to a double once.  Written once for the kernels (the split), the plan (the format) and the
// host result (the conversion), and for the host check (tools/fx_sum_check.cpp).  Needs <math.h> / <stdint.h> only.
//
// Format (E, K, W) of one aggregated column of one plan:
//   E: smallest integer with |v| < 2^E over every finite non-zero operand the plan can read;
//   L: exponent of the lowest set mantissa bit over the same operands (a lower bound serves as well);
//   H = bit_length(total docs of the plan) + 1 bits of headroom, K = 62 - H;
//   W = 2 if E - L <= 2K, else 3;  exact if E - L <= W K, else quantised.
// Split of v: t = ldexp(v, K - E); d0 = trunc(t); t = ldexp(t - d0, K); d1 = trunc(t); ... -- every step exact in
// double arithmetic, every |d| < 2^K, so the sum of fewer than 2^(H - 1) digits stays below 2^61.  The only
// information dropped is what the last trunc of a quantised format cuts off: v truncated toward zero to a multiple of
// 2^(E - W K).
// Result: sum_j D_j 2^((W - 1 - j) K) as one wide integer, rounded to nearest-even once, scaled by 2^(E - W K): in an
// exact format the correctly rounded exact sum.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define PGPU_FX_HD __host__ __device__
#else
#define PGPU_FX_HD
#endif

namespace pgpu {

constexpr int kFxMaxDigits = 3;
enum FxMode : int32_t { FX_NONE = 0, FX_EXACT = 1, FX_QUANTISED = 2 };

struct FxFormat {
  int32_t mode = FX_NONE;
  int32_t E = 0, K = 0, W = 0;
};

// The operands' range: E and L over the finite non-zero values seen so far (any = false: none yet), and whether
// every value was finite.
struct FxRange {
  int32_t E = 0, L = 0;
  bool any = false, finite = true;
};

inline void fx_range_add(FxRange* r, double v) {
  if (!isfinite(v)) { r->finite = false; return; }
  if (v == 0.0) return;
  int e;
  double m = frexp(fabs(v), &e);  // |v| = m 2^e, m in [0.5, 1): |v| < 2^e, and 2^(e - 1) <= |v|
  // lowest set bit: m 2^53 is an integer below 2^53 whose trailing zeros count up from bit e - 53
  uint64_t bits = (uint64_t)ldexp(m, 53);
  const int l = e - 53 + __builtin_ctzll(bits);
  if (!r->any) { r->E = e; r->L = l; r->any = true; return; }
  if (e > r->E) r->E = e;
  if (l < r->L) r->L = l;
}
inline void fx_range_merge(FxRange* r, const FxRange& o) {
  r->finite = r->finite && o.finite;
  if (!o.any) return;
  if (!r->any) { r->E = o.E; r->L = o.L; r->any = true; return; }
  if (o.E > r->E) r->E = o.E;
  if (o.L < r->L) r->L = o.L;
}

// ---- agreement across ranks (pgpu_fp_sum_range, include/pinotgpu.h: the same layout).  Digit sums of different
// formats do not add, so before a cross-GPU query every rank reports, per aggregation, the range of its own operands
// and its docs, the ranks merge what they gathered by the rule below, and every rank plans with the merged ranges
// (pgpu_plan_create_agreed): one (E, K, W) per summed column on every rank, K's headroom over the docs of them all.
struct FxAgree {
  int32_t is_sum = 0;        // 1: SUM / AVG over a numeric column; 0: COUNT / MIN / MAX (the other fields 0)
  int32_t any = 0, finite = 0;  // FxRange.any / .finite
  int32_t E = 0, L = 0;      // FxRange.E / .L (valid when any)
  int32_t reserved = 0;
  int64_t docs = 0;          // documents of the rank's segments
  double int_sum_bound = 0;  // integer columns: sum over segments of numDocs x max |value|, rounded up; else 0
};
// A long double bound as a double that is not below it.
inline double fx_round_up(long double b) {
  double d = (double)b;
  if ((long double)d < b) d = nextafter(d, INFINITY);
  return d;
}
// all[r * num_aggs + a]: rank r's range of aggregation a.  finite: AND; any: OR; E: max, L: min over the ranks with
// any; docs and int_sum_bound: sums.  Returns -1 - a when the ranks differ on is_sum of aggregation a, else 0.
inline int fx_agree_merge(const FxAgree* all, int nranks, int num_aggs, FxAgree* out) {
  for (int a = 0; a < num_aggs; ++a) {
    FxAgree m;
    m.is_sum = all[a].is_sum;
    FxRange r;
    long double bound = 0;
    for (int k = 0; k < nranks; ++k) {
      const FxAgree& x = all[(int64_t)k * num_aggs + a];
      if ((x.is_sum != 0) != (m.is_sum != 0)) return -1 - a;
      if (!x.is_sum) continue;
      FxRange o;
      o.E = x.E;
      o.L = x.L;
      o.any = x.any != 0;
      o.finite = x.finite != 0;
      fx_range_merge(&r, o);
      m.docs += x.docs;
      bound += (long double)x.int_sum_bound;
    }
    if (m.is_sum) {
      m.is_sum = 1;
      m.any = r.any ? 1 : 0;
      m.finite = r.finite ? 1 : 0;
      m.E = r.any ? r.E : 0;
      m.L = r.any ? r.L : 0;
      m.int_sum_bound = fx_round_up(bound);
    }
    out[a] = m;
  }
  return 0;
}

inline int fx_bit_length(int64_t n) {
  int b = 0;
  while (n > 0) { ++b; n >>= 1; }
  return b;
}

// headroom < 0: bit_length(total_docs) + 1 (the plan's); the host check passes 0 to show that the headroom matters.
inline FxFormat fx_format(const FxRange& r, int64_t total_docs, int headroom = -1) {
  FxFormat f;
  if (!r.finite) return f;
  const int H = headroom >= 0 ? headroom : fx_bit_length(total_docs) + 1;
  f.K = 62 - H;
  f.E = r.any ? r.E : 0;
  const int L = r.any ? r.L : 0;
  f.W = f.E - L <= 2 * f.K ? 2 : 3;
  f.mode = f.E - L <= f.W * f.K ? FX_EXACT : FX_QUANTISED;
  return f;
}

// Digit j of v (j < W) in a format with exponent E and K-bit digits, as an integer-valued double of magnitude < 2^K.
// sh = K - E.  v_ldexp_f64 / v_trunc_f64 / v_add_f64 on the device.
PGPU_FX_HD inline double fx_digit_f64(double v, int sh, int K, int j) {
  double t = ldexp(v, sh);
  double d = trunc(t);
  for (int i = 0; i < j; ++i) {
    t = ldexp(t - d, K);
    d = trunc(t);
  }
  return d;
}
PGPU_FX_HD inline int64_t fx_digit(double v, int sh, int K, int j) { return (int64_t)fx_digit_f64(v, sh, K, j); }

// ---- host: the W digit sums -> one double.  The wide integer is kept in four 64-bit limbs (two's complement,
// little-endian): W = 3 digit sums of up to 61 bits at K <= 60 reach 2^181.
struct FxWide {
  uint64_t w[4] = {0, 0, 0, 0};
};
inline void fx_wide_add_shifted(FxWide* a, int64_t v, int shift) {  // a += v 2^shift, 0 <= shift < 128
  uint64_t x[4];
  const uint64_t sign = v < 0 ? ~0ull : 0ull;
  const int limb = shift >> 6, bit = shift & 63;
  for (int i = 0; i < 4; ++i) x[i] = i < limb ? 0ull : sign;
  x[limb] = (uint64_t)v << bit;
  if (limb + 1 < 4) x[limb + 1] = bit ? (uint64_t)((__int128)v >> (64 - bit)) : sign;
  unsigned __int128 carry = 0;
  for (int i = 0; i < 4; ++i) {
    carry += (unsigned __int128)a->w[i] + x[i];
    a->w[i] = (uint64_t)carry;
    carry >>= 64;
  }
}
// The wide integer times 2^scale, rounded to nearest-even once (the scaling is exact: a result in the subnormal range
// is a multiple of 2^-1074 already, see the format's definition).
inline double fx_wide_to_double(const FxWide& a, int scale) {
  uint64_t m[4];
  const bool neg = (a.w[3] >> 63) != 0;
  unsigned __int128 carry = neg ? 1 : 0;
  for (int i = 0; i < 4; ++i) {
    carry += neg ? ~a.w[i] : a.w[i];
    m[i] = (uint64_t)carry;
    carry >>= 64;
  }
  int top = -1;  // highest set bit
  for (int i = 3; i >= 0 && top < 0; --i)
    if (m[i]) top = 64 * i + 63 - __builtin_clzll(m[i]);
  if (top < 0) return 0.0;
  auto bit_at = [&](int b) -> uint64_t { return b < 0 ? 0ull : (m[b >> 6] >> (b & 63)) & 1ull; };
  uint64_t mant = 0;
  int low = top - 52;  // exponent of the mantissa's last bit
  if (low <= 0) {
    mant = m[0];
    low = 0;
  } else {
    for (int b = top; b >= low; --b) mant = (mant << 1) | bit_at(b);
    const uint64_t half = bit_at(low - 1);
    bool sticky = false;
    for (int b = low - 2; b >= 0 && !sticky; --b) sticky = bit_at(b) != 0;
    if (half && (sticky || (mant & 1ull))) ++mant;  // 2^53 after the carry is exact as a double too
  }
  const double r = ldexp((double)mant, low + scale);
  return neg ? -r : r;
}
// digits[j] = sum over the docs of digit j.
inline double fx_result(const int64_t* digits, const FxFormat& f) {
  FxWide a;
  for (int j = 0; j < f.W; ++j) fx_wide_add_shifted(&a, digits[j], (f.W - 1 - j) * f.K);
  return fx_wide_to_double(a, f.E - f.W * f.K);
}

}  // namespace pgpu
