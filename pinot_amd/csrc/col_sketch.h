// col_sketch.h -- byte-code sketches of wide dictionary filter columns: the code assignment and the exactness tests.
// Pure host code over plain vectors (no device, no table type), shared by the pin-time builder (rt_sketch.cpp), the
// planner (rt_plan_create.cpp) and the stand-alone checker (tools/col_sketch_check.cpp).
//
// A sketch maps every dictId of one segment's column to one of at most 256 codes, monotone non-decreasing in the
// dictId, so that every code is an interval [first_id[c], first_id[c + 1]) of dictIds:
//   - up to kSketchHot (127) hot dictIds -- the largest doc counts, ties to the lower dictId, counts > 0 only -- get a
//     code of their own (a singleton);
//   - every non-empty gap between hot ids, before the first and after the last, is one interval code.
// 127 singletons and at most 128 gaps make at most 255 codes.  The per-doc codes are a second, 8-bit forward index of
// the column; a predicate may be evaluated on it instead of the dictIds only where the codes answer it exactly:
//   - a dictId range [lo, hi) whose two ends are code boundaries, as the code range [code(lo), code(hi));
//   - a dictId set that holds every code's interval wholly or not at all, as a set of codes.
// Match masks are then bit for bit those of the dictId scan: no verification pass, the same statistics.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pgpu {

constexpr int kSketchHot = 127;
constexpr int kSketchMaxCodes = 256;
constexpr int kSketchBits = 8;
constexpr int kSketchSetWords = kSketchMaxCodes / 32;

struct ColSketch {
  int32_t card = 0;
  int32_t ncodes = 0;              // 0: no sketch
  std::vector<int32_t> first_id;   // [ncodes + 1], first_id[ncodes] = card
  std::vector<uint8_t> singleton;  // [ncodes]: 1 = the code of one hot dictId
  std::vector<uint8_t> lut;        // [card]: dictId -> code
  int64_t singleton_docs = 0;      // docs whose dictId has a singleton code
  int64_t total_docs = 0;
  // code(card) = ncodes: the end of the last code
  int code(int64_t id) const { return id >= card ? ncodes : (int)lut[id]; }
};

// The assignment from the column's per-dictId doc counts.
template <typename Count>
inline void sketch_assign(const Count* counts, int32_t card, ColSketch* out) {
  ColSketch& s = *out;
  s = ColSketch();
  if (card <= 0) return;
  s.card = card;
  std::vector<int32_t> hot;
  for (int32_t i = 0; i < card; ++i) {
    s.total_docs += (int64_t)counts[i];
    if (counts[i] > 0) hot.push_back(i);
  }
  auto hotter = [&](int32_t a, int32_t b) { return counts[a] != counts[b] ? counts[a] > counts[b] : a < b; };
  if ((int)hot.size() > kSketchHot) {
    std::nth_element(hot.begin(), hot.begin() + kSketchHot, hot.end(), hotter);
    hot.resize(kSketchHot);
  }
  std::sort(hot.begin(), hot.end());
  s.lut.assign((size_t)card, 0);
  int32_t next = 0;  // first dictId without a code
  auto close_gap = [&](int32_t end) {
    if (end <= next) return;
    std::fill(s.lut.begin() + next, s.lut.begin() + end, (uint8_t)s.first_id.size());
    s.first_id.push_back(next);
    s.singleton.push_back(0);
    next = end;
  };
  for (int32_t h : hot) {
    close_gap(h);
    s.lut[h] = (uint8_t)s.first_id.size();
    s.first_id.push_back(h);
    s.singleton.push_back(1);
    s.singleton_docs += (int64_t)counts[h];
    next = h + 1;
  }
  close_gap(card);
  s.ncodes = (int32_t)s.first_id.size();
  s.first_id.push_back(card);
}

// dictId range [lo, hi), 0 <= lo < hi <= card: exact on the sketch iff both ends are code boundaries; then it is the
// code range [*clo, *chi).
inline bool sketch_range_exact(const ColSketch& s, int64_t lo, int64_t hi, int* clo, int* chi) {
  if (s.ncodes <= 0 || lo < 0 || lo >= hi || hi > s.card) return false;
  const int a = s.code(lo), b = s.code(hi);
  if (s.first_id[a] != lo) return false;
  if (hi != s.card && s.first_id[b] != hi) return false;
  *clo = a;
  *chi = b;
  return true;
}

// Bits [a, b) of a bitset of 32-bit words that are set.
inline int64_t sketch_bits_set(const uint32_t* w, int64_t a, int64_t b) {
  int64_t n = 0;
  while (a < b) {
    const int sh = (int)(a & 31);
    const int64_t take = std::min<int64_t>(32 - sh, b - a);
    uint32_t x = w[a >> 5] >> sh;
    if (take < 32) x &= (1u << take) - 1u;
    n += __builtin_popcount(x);
    a += take;
  }
  return n;
}

// dictId set (bit i of word i >> 5 = dictId i, ceil(card / 32) words): exact on the sketch iff every code's interval is
// wholly inside or wholly outside the set; then codes[] (kSketchSetWords words) is the set of the codes inside.
inline bool sketch_set_exact(const ColSketch& s, const uint32_t* set, uint32_t* codes) {
  if (s.ncodes <= 0) return false;
  for (int k = 0; k < kSketchSetWords; ++k) codes[k] = 0;
  for (int c = 0; c < s.ncodes; ++c) {
    const int64_t a = s.first_id[c], b = s.first_id[c + 1];
    const int64_t n = sketch_bits_set(set, a, b);
    if (n == b - a) codes[c >> 5] |= 1u << (c & 31);
    else if (n != 0) return false;
  }
  return true;
}

}  // namespace pgpu
