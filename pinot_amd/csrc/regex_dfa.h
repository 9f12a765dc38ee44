// regex_dfa.h -- REGEXP_LIKE / LIKE over a string dictionary: the accepted subset of java.util.regex compiled into a
// DFA (regex_dfa.cpp).  Plain C++, no HIP: it compiles into a stand-alone host program (tools/regex_fuzz.cpp).
//
// The reference evaluates Pattern.compile(p, CASE_INSENSITIVE | UNICODE_CASE).matcher(value).find()
// (RegexpLikePredicateEvaluatorFactory.java:64-80).  The subset is the part of that language whose meaning is
// unambiguous and coincides with a textbook automaton over ASCII values without line terminators (include/pinotgpu.h,
// PGPU_PRED_REGEXP_LIKE, lists it and every declined shape); anything else is declined with a message, never
// approximated.
//
// The automaton reads `value EOS`: find() is the search prefix X* in front of the pattern, `^` holds only before the
// first byte (the start state is the state after the begin-of-input), `$` only at EOS.  Accepting is absorbing -- one
// accepting state, row 0 of the table -- because find() asks for any match.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pgpu {

constexpr int kRegexMaxPattern = 1024;         // bytes of pattern text
constexpr int kRegexMaxRepeat = 64;            // the largest bound of {n}, {n,}, {n,m}
constexpr int kRegexMaxTableBytes = 32 * 1024; // states x classes x 2: the kernel's LDS table (PGPU_REGEX_MAX_TABLE_BYTES)
constexpr int kRegexEos = 256;                 // the end-of-input symbol, after the 256 byte values
constexpr int kRegexSymbols = 257;
constexpr int kRegexClsBytes = 264;            // the class map padded to a multiple of 8 bytes

struct RegexDfa {
  int32_t num_states = 0, num_classes = 0;
  uint8_t cls[kRegexClsBytes] = {};  // input symbol -> equivalence class
  // table[state * num_classes + class] = next state * num_classes: the row offset itself, so that a step is one add and
  // one load.  State 0 is the accepting state (every entry of row 0 is 0).
  std::vector<uint16_t> table;
  uint16_t start_row = 0;            // the state after begin-of-input, as a row offset
  int64_t table_bytes() const { return (int64_t)table.size() * 2; }
};

// Compiles pattern[0, len).  Returns 0, or 1 with *err naming what was met (a construct outside the subset, or a table
// past kRegexMaxTableBytes).
int regex_compile(const char* pattern, size_t len, RegexDfa* out, std::string* err);

// The host interpreter of the same table: Matcher.find() on value[0, n).
bool regex_match(const RegexDfa& d, const uint8_t* value, size_t n);

// True when the value is inside the limit the exactness rule sets: ASCII, no \n, no \r.
inline bool regex_value_ok(const uint8_t* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (v[i] >= 0x80 || v[i] == 0x0A || v[i] == 0x0D) return false;
  return true;
}

}  // namespace pgpu
