// key_range_check.cpp -- host check of the key range a rank owns in the dense cross-GPU combine
// (pinot_amd/csrc/key_range.h: owned_key_range; nothing else of the library is included or linked).  Built under
// AddressSanitizer + UndefinedBehaviorSanitizer by pinot_amd.build.build_key_range_check, run by
// tests/test_distinct_combine_cpu.py, which pins the printed ranges against plain Python.
//
// Usage: key_range_check G N [G N ...] -- one line "G N rank chunk begin count" per rank of every pair.
#include <cstdio>
#include <cstdlib>

#include "key_range.h"

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2) {
    fprintf(stderr, "usage: %s G N [G N ...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 1 < argc; i += 2) {
    const long long G = atoll(argv[i]);
    const int N = atoi(argv[i + 1]);
    for (int r = 0; r < N; ++r) {
      const pgpu::KeyRange k = pgpu::owned_key_range(G, N, r);
      printf("%lld %d %d %lld %lld %lld\n", G, N, r, (long long)k.chunk, (long long)k.begin, (long long)k.count);
    }
  }
  return 0;
}
