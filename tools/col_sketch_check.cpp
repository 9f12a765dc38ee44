// col_sketch_check.cpp -- host check of the byte-code sketches of filter columns (pinot_amd/csrc/col_sketch.h, the
// header the pin-time builder and the planner share; nothing else of the library is included or linked).  Built under
// AddressSanitizer + UndefinedBehaviorSanitizer by pinot_amd.build.build_col_sketch_check, run by
// tests/test_col_sketch_cpu.py.
//
// Over random and adversarial doc histograms (cardinalities 1, 255, 256, 257, 2049, 100 000; all counts equal; all mass
// on the first / last dictId; adjacent hot ids; more than 127 tied candidates; zero-count ids):
//   codes      at most 256, monotone non-decreasing in the dictId, first_id consistent with the dictId -> code table;
//   singletons exactly the ids an independent selection picks (largest count, ties to the lower id, counts > 0 only,
//              at most 127), and their docs summed;
//   ranges     for every [lo, hi) of a small cardinality, and random ones of a large one: sketch_range_exact says yes
//              iff the dictIds the code range selects are the range's;
//   sets       the same for random dictId sets, built to be exact, nearly exact and arbitrary.
// Exit status 0 = all held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "col_sketch.h"

using namespace pgpu;

static long long g_cases = 0, g_failures = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;

static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

static void failure(const char* name, const char* what, long long a, long long b) {
  if (++g_failures <= 40) printf("FAIL %s: %s: %lld vs %lld\n", name, what, a, b);
}

// the dictIds a code range / code set selects, as a per-dictId flag vector
static std::vector<uint8_t> select_codes(const ColSketch& s, const uint32_t* codes) {
  std::vector<uint8_t> sel((size_t)s.card, 0);
  for (int32_t i = 0; i < s.card; ++i) sel[i] = (codes[s.lut[i] >> 5] >> (s.lut[i] & 31)) & 1u;
  return sel;
}

static void check_structure(const char* name, const std::vector<uint32_t>& cnt, const ColSketch& s) {
  const int32_t card = (int32_t)cnt.size();
  if (s.card != card) failure(name, "card", s.card, card);
  if (s.ncodes < 1 || s.ncodes > kSketchMaxCodes) failure(name, "ncodes", s.ncodes, kSketchMaxCodes);
  if ((int)s.first_id.size() != s.ncodes + 1 || (int)s.singleton.size() != s.ncodes || (int)s.lut.size() != card) {
    failure(name, "vector sizes", (long long)s.first_id.size(), s.ncodes + 1);
    return;
  }
  if (s.first_id[0] != 0) failure(name, "first_id[0]", s.first_id[0], 0);
  if (s.first_id[s.ncodes] != card) failure(name, "first_id[ncodes]", s.first_id[s.ncodes], card);
  for (int c = 0; c < s.ncodes; ++c)
    if (s.first_id[c] >= s.first_id[c + 1]) failure(name, "empty or unordered code", c, s.first_id[c]);
  for (int32_t i = 0; i < card; ++i) {
    const int c = s.lut[i];
    if (i > 0 && c < s.lut[i - 1]) failure(name, "not monotone at", i, c);
    if (c >= s.ncodes || i < s.first_id[c] || i >= s.first_id[c + 1]) failure(name, "lut outside its code at", i, c);
  }
  if (s.code(card) != s.ncodes) failure(name, "code(card)", s.code(card), s.ncodes);
  // the hot ids, selected independently: a full sort by (count descending, id ascending)
  std::vector<int32_t> order;
  int64_t total = 0;
  for (int32_t i = 0; i < card; ++i) {
    total += cnt[i];
    if (cnt[i] > 0) order.push_back(i);
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cnt[a] > cnt[b]; });
  if ((int)order.size() > kSketchHot) order.resize(kSketchHot);
  std::vector<uint8_t> hot((size_t)card, 0);
  int64_t hot_docs = 0;
  for (int32_t i : order) {
    hot[i] = 1;
    hot_docs += cnt[i];
  }
  for (int32_t i = 0; i < card; ++i) {
    const int c = s.lut[i];
    const bool single = s.singleton[c] != 0;
    if (single != (hot[i] != 0)) failure(name, "singleton flag differs from the selection at", i, single);
    if (single && s.first_id[c + 1] - s.first_id[c] != 1) failure(name, "singleton code of several ids", c, i);
    // a gap never spans a hot id: its neighbours in the same code are all cold (checked through the flag above)
  }
  if (s.singleton_docs != hot_docs) failure(name, "singleton_docs", s.singleton_docs, hot_docs);
  if (s.total_docs != total) failure(name, "total_docs", s.total_docs, total);
}

static void check_range(const char* name, const ColSketch& s, int64_t lo, int64_t hi) {
  ++g_cases;
  int a = -1, b = -1;
  const bool exact = sketch_range_exact(s, lo, hi, &a, &b);
  // ground truth: [lo, hi) is a union of whole codes
  bool truth = true;
  for (int c = 0; c < s.ncodes && truth; ++c) {
    const int64_t f = s.first_id[c], e = s.first_id[c + 1];
    const int64_t in = std::max<int64_t>(0, std::min(e, hi) - std::max(f, lo));
    truth = in == 0 || in == e - f;
  }
  if (exact != truth) {
    failure(name, "range exactness", lo, hi);
    return;
  }
  if (!exact) return;
  if (a < 0 || b <= a || b > s.ncodes) {
    failure(name, "code range", a, b);
    return;
  }
  if (s.first_id[a] != lo || s.first_id[b] != hi) failure(name, "code range selects other dictIds", lo, hi);
}

static void check_set(const char* name, const ColSketch& s, const std::vector<uint32_t>& set) {
  ++g_cases;
  uint32_t codes[kSketchSetWords];
  const bool exact = sketch_set_exact(s, set.data(), codes);
  bool truth = true;
  for (int c = 0; c < s.ncodes && truth; ++c) {
    int64_t in = 0;
    for (int32_t i = s.first_id[c]; i < s.first_id[c + 1]; ++i) in += (set[i >> 5] >> (i & 31)) & 1u;
    truth = in == 0 || in == s.first_id[c + 1] - s.first_id[c];
  }
  if (exact != truth) {
    failure(name, "set exactness", exact, truth);
    return;
  }
  if (!exact) return;
  const std::vector<uint8_t> sel = select_codes(s, codes);
  for (int32_t i = 0; i < s.card; ++i)
    if (sel[i] != ((set[i >> 5] >> (i & 31)) & 1u)) {
      failure(name, "code set selects other dictIds at", i, sel[i]);
      return;
    }
  for (int c = s.ncodes; c < kSketchMaxCodes; ++c)
    if ((codes[c >> 5] >> (c & 31)) & 1u) failure(name, "code past ncodes set", c, s.ncodes);
}

static void check_histogram(const char* name, const std::vector<uint32_t>& cnt) {
  const int32_t card = (int32_t)cnt.size();
  ColSketch s;
  sketch_assign(cnt.data(), card, &s);
  check_structure(name, cnt, s);
  if (g_failures) return;
  if (card <= 300) {
    for (int64_t lo = 0; lo < card; ++lo)
      for (int64_t hi = lo + 1; hi <= card; ++hi) check_range(name, s, lo, hi);
  } else {
    for (int k = 0; k < 20000; ++k) {
      int64_t lo, hi;
      switch (k & 3) {
        case 0:  // both ends on code boundaries
          lo = s.first_id[rnd() % s.ncodes];
          hi = s.first_id[1 + rnd() % s.ncodes];
          break;
        case 1:  // one end moved by one dictId
          lo = s.first_id[rnd() % s.ncodes] + (int64_t)(rnd() % 3) - 1;
          hi = s.first_id[1 + rnd() % s.ncodes] + (int64_t)(rnd() % 3) - 1;
          break;
        case 2:  // a single dictId
          lo = (int64_t)(rnd() % card);
          hi = lo + 1;
          break;
        default:
          lo = (int64_t)(rnd() % card);
          hi = (int64_t)(rnd() % (card + 1));
      }
      if (lo < 0 || lo >= hi || hi > card) continue;
      check_range(name, s, lo, hi);
    }
  }
  // out-of-domain ranges are never exact
  int a, b;
  if (sketch_range_exact(s, 0, 0, &a, &b) || sketch_range_exact(s, -1, 1, &a, &b) ||
      sketch_range_exact(s, 0, (int64_t)card + 1, &a, &b))
    failure(name, "out-of-domain range accepted", 0, card);
  const size_t words = ((size_t)card + 31) / 32;
  const int nsets = card <= 300 ? 300 : 60;
  for (int k = 0; k < nsets; ++k) {
    std::vector<uint32_t> set(words, 0u);
    auto put = [&](int64_t i) { set[i >> 5] |= 1u << (i & 31); };
    if (k % 3 != 2) {  // a union of whole codes ...
      for (int c = 0; c < s.ncodes; ++c)
        if (rnd() & 1)
          for (int32_t i = s.first_id[c]; i < s.first_id[c + 1]; ++i) put(i);
      if (k % 3 == 1) set[(rnd() % card) >> 5] ^= 1u << (rnd() & 31);  // ... with one bit flipped (spare bits too)
      if (card & 31) set[words - 1] &= (1u << (card & 31)) - 1u;
    } else {
      const int n = 1 + (int)(rnd() % 8);
      for (int j = 0; j < n; ++j) put((int64_t)(rnd() % card));
    }
    check_set(name, s, set);
  }
}

int main() {
  const int32_t cards[] = {1, 255, 256, 257, 2049, 100000};
  for (int32_t card : cards) {
    char name[96];
    std::vector<uint32_t> cnt((size_t)card);
    auto run = [&](const char* what) {
      snprintf(name, sizeof name, "card %d, %s", card, what);
      check_histogram(name, cnt);
    };
    std::fill(cnt.begin(), cnt.end(), 7u);
    run("all counts equal");  // more than 127 tied candidates where card > 127
    std::fill(cnt.begin(), cnt.end(), 0u);
    run("no docs");
    cnt[0] = 1000000u;
    run("all mass on id 0");
    cnt[0] = 0u;
    cnt[card - 1] = 1000000u;
    run("all mass on the last id");
    for (int32_t i = 0; i < card; ++i) cnt[i] = (uint32_t)(1000000.0 / (1 + i));  // Zipf by dictId: adjacent hot ids
    run("adjacent hot ids at the front");
    std::reverse(cnt.begin(), cnt.end());
    run("adjacent hot ids at the back");
    for (int32_t i = 0; i < card; ++i) cnt[i] = (i % 3 == 0) ? 5u : 0u;  // ties and zero-count ids interleaved
    run("every third id, tied");
    for (int32_t i = 0; i < card; ++i) cnt[i] = (i & 1) ? 9u : 8u;  // 127 cut inside a tie
    run("two tied levels");
    for (int rep = 0; rep < 6; ++rep) {
      for (int32_t i = 0; i < card; ++i) {
        const uint64_t r = rnd();
        const uint32_t heavy = (r % 97 == 0) ? (uint32_t)(rnd() % 100000) : 0u;
        cnt[i] = (r & 4) ? 0u : (uint32_t)((r >> 8) % 50) + heavy;
      }
      run("random, sparse heavy hitters");
    }
    for (int rep = 0; rep < 3; ++rep) {  // Zipf over a random permutation of the ids, as the workload's account ids
      std::vector<int32_t> perm((size_t)card);
      for (int32_t i = 0; i < card; ++i) perm[i] = i;
      for (int32_t i = card - 1; i > 0; --i) std::swap(perm[i], perm[rnd() % (i + 1)]);
      for (int32_t i = 0; i < card; ++i) cnt[perm[i]] = (uint32_t)(1000000.0 / (1 + i));
      run("Zipf over shuffled ids");
    }
  }
  ColSketch none;
  sketch_assign((const uint32_t*)nullptr, 0, &none);
  if (none.ncodes != 0) failure("card 0", "ncodes", none.ncodes, 0);
  printf("%lld range / set cases, %lld failures\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
