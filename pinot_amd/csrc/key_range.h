// key_range.h — the key range a rank owns in the dense cross-GPU combine (pgpu_plan_combine): the rows of the group
// table are reduce-scattered by it (PGPU_COMBINE_REDUCE_SCATTER), and the DISTINCTCOUNT side bitmaps are exchanged and
// merged by it in both dense modes.  One header, so the two splits cannot drift apart; it includes nothing of the
// library (tools/key_range_check.cpp pins it against plain arithmetic on the host).
#pragma once
#include <cstdint>

namespace pgpu {

struct KeyRange {
  int64_t chunk = 0;  // ceil(num_keys / nranks): the keys of every rank but the last non-empty one
  int64_t begin = 0;
  int64_t count = 0;
};

// Rank `rank` of `nranks` owns keys [min(G, rank * chunk), min(G, (rank + 1) * chunk)): ordered by rank, disjoint,
// together all of [0, G); ranks past the keys (G < nranks) own none.
inline KeyRange owned_key_range(int64_t num_keys, int nranks, int rank) {
  KeyRange r;
  if (num_keys <= 0 || nranks <= 0 || rank < 0) return r;
  r.chunk = (num_keys + nranks - 1) / nranks;
  // (rank * chunk stays below 2^63: chunk <= num_keys, and a rank past the keys is clamped before the product)
  r.begin = (int64_t)rank >= (num_keys + r.chunk - 1) / r.chunk ? num_keys : (int64_t)rank * r.chunk;
  const int64_t end = num_keys - r.begin < r.chunk ? num_keys : r.begin + r.chunk;
  r.count = end - r.begin;
  return r;
}

}  // namespace pgpu
