// regex_fuzz.cpp -- a stand-alone host program over pinot_amd/csrc/regex_dfa.cpp alone, built with AddressSanitizer and
// UndefinedBehaviorSanitizer (pinot_amd.build.build_regex_fuzz).  It compiles random byte strings, mutated and truncated
// seed patterns, and runs every automaton that compiles over random and truncated values, checking the blob's
// invariants on the way: every entry a row offset inside the table, row 0 absorbing, the table within its cap, a
// declined pattern always with a message.  No device code, no library.
//
//   regex_fuzz [iterations] [seed]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "regex_dfa.h"

using namespace pgpu;

static uint64_t g_state = 1;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

static const char* kSeeds[] = {
    "^foo.*bar$", "(a|b)*abb", "[a-z0-9_]+@[a-z]+\\.com", "a{2,3}$", "(^a|b$)", "[^a-c\\d-]x?", "\\w+\\s\\W\\D\\S",
    "(?:ab|cd){1,4}e*", "^$", "a^b", "x{64}", "(a|b)*a(a|b){12}", "[\\d-]", "\\<\\>\\-\\&\\/", "(|a)(b|)", "((((a))))+",
    "^.*\\.html$", "[A-Z][a-z]{0,8}", "a{3,}b{0,2}", "[-a]|[a-]|[\\^x^]",
};
static const char kMeta[] = "\\^$.{}[]()*+?|<>-&/,:0123456789abAZz_ \t";

static std::string random_pattern() {
  const int kind = below(4);
  std::string s;
  if (kind == 0) {  // raw bytes
    const int n = below(24);
    for (int i = 0; i < n; ++i) s.push_back((char)below(256));
  } else if (kind == 1) {  // metacharacter soup
    const int n = below(32);
    for (int i = 0; i < n; ++i) s.push_back(kMeta[below((int)sizeof(kMeta) - 1)]);
  } else {  // a seed, truncated and / or mutated
    s = kSeeds[below((int)(sizeof(kSeeds) / sizeof(kSeeds[0])))];
    if (kind == 3 && !s.empty()) s.resize(below((int)s.size() + 1));
    const int muts = below(3);
    for (int m = 0; m < muts && !s.empty(); ++m) {
      const int at = below((int)s.size());
      switch (below(3)) {
        case 0: s[at] = kMeta[below((int)sizeof(kMeta) - 1)]; break;
        case 1: s.insert(s.begin() + at, kMeta[below((int)sizeof(kMeta) - 1)]); break;
        default: s.erase(s.begin() + at); break;
      }
    }
  }
  return s;
}

static int check_blob(const RegexDfa& d, const std::string& pat) {
  const size_t want = (size_t)d.num_states * (size_t)d.num_classes;
  if (d.num_states < 1 || d.num_classes < 2 || d.table.size() != want || d.table_bytes() > kRegexMaxTableBytes ||
      d.start_row >= want || d.start_row % d.num_classes) {
    fprintf(stderr, "bad blob shape for pattern of %zu bytes\n", pat.size());
    return 1;
  }
  for (int s = 0; s < kRegexSymbols; ++s)
    if (d.cls[s] >= d.num_classes) { fprintf(stderr, "class out of range\n"); return 1; }
  for (size_t k = 0; k < want; ++k)
    if (d.table[k] >= want || d.table[k] % d.num_classes || (k < (size_t)d.num_classes && d.table[k] != 0)) {
      fprintf(stderr, "bad table entry %zu\n", k);
      return 1;
    }
  return 0;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 20000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345;
  long compiled = 0, declined = 0, matches = 0;
  // the length limit, from both sides
  {
    RegexDfa d;
    std::string err;
    const std::string at(kRegexMaxPattern, 'a'), over(kRegexMaxPattern + 1, 'a');
    if (regex_compile(at.data(), at.size(), &d, &err) != 0 || regex_compile(over.data(), over.size(), &d, &err) != 1) {
      fprintf(stderr, "pattern length limit\n");
      return 1;
    }
  }
  for (long it = 0; it < iters; ++it) {
    const std::string pat = random_pattern();
    RegexDfa d;
    std::string err;
    const int rc = regex_compile(pat.data(), pat.size(), &d, &err);
    if (rc != 0) {
      if (rc != 1 || err.empty()) { fprintf(stderr, "decline without a message\n"); return 1; }
      ++declined;
      continue;
    }
    ++compiled;
    if (check_blob(d, pat)) return 1;
    for (int v = 0; v < 8; ++v) {
      std::vector<uint8_t> val((size_t)below(40));
      for (auto& b : val) b = (uint8_t)(below(4) ? "abz09_A. /<"[below(11)] : below(256));
      // a heap copy of the exact length: a read past the value is the sanitizer's to report
      uint8_t* heap = (uint8_t*)malloc(val.size() ? val.size() : 1);
      if (!val.empty()) memcpy(heap, val.data(), val.size());
      const bool whole = regex_match(d, heap, val.size());
      matches += whole;
      if (!val.empty()) matches += regex_match(d, heap, val.size() / 2);  // truncated
      (void)regex_value_ok(heap, val.size());
      free(heap);
    }
  }
  printf("regex_fuzz ok: %ld patterns compiled, %ld declined, %ld matches\n", compiled, declined, matches);
  return 0;
}
