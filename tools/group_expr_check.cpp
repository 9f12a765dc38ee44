// group_expr_check -- the host steps of a derived column's build (pinot_amd/csrc/group_expr.h: sort-unique of the
// candidate keys, compaction of the used candidates into the typed dictionary, the candidate -> dictId remap, the bit
// width) as a stand-alone program, so that they run under AddressSanitizer + UndefinedBehaviorSanitizer without a GPU
// (pinot_amd.build.build_group_expr_check).  It plays the kernels' part on the host: keys by expr_value_key, a doc's
// candidate by binary search, the candidate marked used.
//
// stdin, one case after another:
//   build <type 0..3> <ncand> <ndocs>
//   <ncand values: the candidates' doubles as 16 hex digits each, any order, duplicates allowed>
//   <ndocs values: the docs' doubles; each must be among the candidates>
// stdout per case:
//   card <card> bits <bits> width <entry_width> cand <unique candidates>
//   dict <the dictionary's bytes in hex>
//   remap <one entry per unique candidate, -1 for an unused one>
//   ids <the docs' local dictIds>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "expr_eval.h"
#include "group_expr.h"

using namespace pgpu;

static bool read_double(double* out) {
  char buf[64];
  if (scanf("%63s", buf) != 1) return false;
  const uint64_t u = strtoull(buf, nullptr, 16);
  memcpy(out, &u, 8);
  return true;
}

int main() {
  char word[32];
  while (scanf("%31s", word) == 1) {
    if (std::string(word) != "build") {
      fprintf(stderr, "unknown command %s\n", word);
      return 2;
    }
    int type = 0;
    long ncand = 0, ndocs = 0;
    if (scanf("%d %ld %ld", &type, &ncand, &ndocs) != 3 || type < 0 || type > 3 || ncand < 0 || ndocs < 0) {
      fprintf(stderr, "bad build line\n");
      return 2;
    }
    std::vector<int64_t> cand;
    for (long i = 0; i < ncand; ++i) {
      double d;
      if (!read_double(&d)) return 2;
      cand.push_back(expr_value_key(d));
    }
    group_expr_sort_unique(&cand);
    std::vector<uint32_t> used(cand.size(), 0u), scratch;
    for (long i = 0; i < ndocs; ++i) {
      double d;
      if (!read_double(&d)) return 2;
      const int64_t key = expr_value_key(d);
      const size_t a = (size_t)(std::lower_bound(cand.begin(), cand.end(), key) - cand.begin());
      if (a >= cand.size() || cand[a] != key) {
        fprintf(stderr, "doc %ld: its value is no candidate\n", i);
        return 2;
      }
      scratch.push_back((uint32_t)a);
      used[a] = 1u;
    }
    const GroupExprDict d = group_expr_compact(cand, used, type);
    printf("card %d bits %d width %d cand %zu\ndict ", d.card, d.bits, d.entry_width, cand.size());
    for (uint8_t b : d.bytes) printf("%02x", b);
    printf("\nremap");
    for (int32_t r : d.remap) printf(" %d", r);
    printf("\nids");
    for (uint32_t s : scratch) printf(" %d", d.remap[s]);
    printf("\n");
  }
  return 0;
}
