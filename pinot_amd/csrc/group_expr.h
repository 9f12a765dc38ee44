// group_expr.h -- host side of the derived columns of group-by expressions (GROUP BY a + b: pgpu_table_add_group_expression):
// what happens between the kernels that build one (k_derive.hip).  The candidate keys come back from the device as
// expr_value_key words (expr_eval.h: the order-preserving int64 of the evaluator's double, every NaN one key); here they
// are sorted and made unique, the candidates a doc used become the dictionary -- sorted, only values present, typed by
// the expression's result type -- and the candidate -> local dictId remap and the bit width follow.  Plain host code
// over the standard library, so rt_dict.cpp and tools/group_expr_check.cpp share it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace pgpu {

// The data types of include/pinotgpu.h (PGPU_INT .. PGPU_DOUBLE), restated so that the header stands alone.
enum GroupExprType : int32_t { GX_INT = 0, GX_LONG = 1, GX_FLOAT = 2, GX_DOUBLE = 3 };

// Step 1: the candidate keys in key order, each once.
inline void group_expr_sort_unique(std::vector<int64_t>* keys) {
  std::sort(keys->begin(), keys->end());
  keys->erase(std::unique(keys->begin(), keys->end()), keys->end());
}

// The double behind a key (the inverse of double_key_bits).
inline double group_expr_key_double(int64_t k) {
  const int64_t b = k >= 0 ? k : (k ^ INT64_MAX);
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// PinotDataBitSet.getNumBitsPerValue of the largest dictId: bit length, at least 1.
inline int group_expr_bits(int32_t card) {
  int max_value = card - 1, n = 0;
  if (max_value <= 1) return 1;
  while (max_value) { n++; max_value >>= 1; }
  return n;
}

// A derived column's dictionary as compacted from the candidates.
struct GroupExprDict {
  std::vector<int64_t> keys;     // the used candidates' keys, ascending: local dictId -> key
  std::vector<int32_t> remap;    // candidate index -> local dictId, -1 for a candidate no doc used
  std::vector<int64_t> iv;       // INT / LONG: the values
  std::vector<double> dv;        // FLOAT / DOUBLE: the values ((double)(float) of a FLOAT one)
  std::vector<uint8_t> bytes;    // the dictionary file's entries: big-endian, 4 (INT, FLOAT) or 8 (LONG, DOUBLE) bytes each
  int32_t card = 0, bits = 1, entry_width = 8;
};

// Step 3: the used candidates (used[i] != 0; cand sorted and unique) become the dictionary of type `type`.  The order of
// the keys is the order of the typed values: an INT / LONG value is the integer the double holds, a FLOAT value the
// float it holds.
inline GroupExprDict group_expr_compact(const std::vector<int64_t>& cand, const std::vector<uint32_t>& used, int32_t type) {
  GroupExprDict d;
  d.remap.assign(cand.size(), -1);
  for (size_t i = 0; i < cand.size(); ++i)
    if (i < used.size() && used[i]) {
      d.remap[i] = (int32_t)d.keys.size();
      d.keys.push_back(cand[i]);
    }
  d.card = (int32_t)d.keys.size();
  d.bits = group_expr_bits(d.card);
  d.entry_width = (type == GX_INT || type == GX_FLOAT) ? 4 : 8;
  d.bytes.assign((size_t)d.card * d.entry_width, 0);
  auto be = [](uint8_t* o, uint64_t v, int w) {
    for (int k = 0; k < w; ++k) o[k] = (uint8_t)(v >> (8 * (w - 1 - k)));
  };
  for (int32_t i = 0; i < d.card; ++i) {
    const double v = group_expr_key_double(d.keys[i]);
    uint8_t* o = d.bytes.data() + (size_t)i * d.entry_width;
    if (type == GX_INT || type == GX_LONG) {
      // (a NaN or a value past the type's range cannot come from an INT / LONG typed program over checked operands; it is
      // clamped rather than left to an undefined conversion)
      const int64_t x = v != v ? 0 : v >= 9223372036854775807.0 ? INT64_MAX : v <= -9223372036854775808.0 ? INT64_MIN : (int64_t)v;
      d.iv.push_back(x);
      if (type == GX_INT) be(o, (uint64_t)(uint32_t)(int32_t)x, 4);
      else be(o, (uint64_t)x, 8);
    } else if (type == GX_FLOAT) {
      const float f = (float)v;
      uint32_t u;
      memcpy(&u, &f, 4);
      d.dv.push_back((double)f);
      be(o, u, 4);
    } else {
      uint64_t u;
      memcpy(&u, &v, 8);
      d.dv.push_back(v);
      be(o, u, 8);
    }
  }
  return d;
}

}  // namespace pgpu
