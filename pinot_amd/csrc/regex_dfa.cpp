// regex_dfa.cpp -- parse -> NFA -> subset construction -> byte-class compression (regex_dfa.h).  Plain C++.
#include "regex_dfa.h"

#include <algorithm>
#include <bitset>
#include <cstdio>
#include <cstring>
#include <map>

namespace pgpu {
namespace {

using ByteSet = std::bitset<256>;

constexpr int kMaxDepth = 200;          // nested groups
constexpr int kMaxNfaStates = 1 << 15;  // after the counted repeats are unrolled
constexpr int64_t kMaxWork = 1 << 26;   // NFA states visited by the subset construction

bool is_digit(int c) { return c >= '0' && c <= '9'; }
bool is_lower(int c) { return c >= 'a' && c <= 'z'; }
bool is_upper(int c) { return c >= 'A' && c <= 'Z'; }
bool is_alnum(int c) { return is_digit(c) || is_lower(c) || is_upper(c); }

// CASE_INSENSITIVE over ASCII: a letter brings its other case
void fold_case(ByteSet& s) {
  for (int k = 0; k < 26; ++k)
    if (s['a' + k] || s['A' + k]) s['a' + k] = s['A' + k] = true;
}

// \d \w \s and their complements over the 256 byte values (Java's default, ASCII, meanings)
bool shorthand(int c, ByteSet* out) {
  ByteSet s;
  switch (c | 0x20) {
    case 'd': for (int b = '0'; b <= '9'; ++b) s[b] = true; break;
    case 'w':
      for (int b = 0; b < 128; ++b) s[b] = is_alnum(b) || b == '_';
      break;
    case 's': for (int b : {0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D}) s[b] = true; break;
    default: return false;
  }
  *out = is_upper(c) ? ~s : s;
  return true;
}

struct Node {
  enum Kind { EMPTY, SET, BOL, EOL, CAT, ALT, REP } kind = EMPTY;
  int set = -1;        // SET: index into Parser::sets
  int lo = 0, hi = 0;  // REP: hi < 0 is unbounded
  std::vector<int> kids;
};

struct Parser {
  const uint8_t* p;
  size_t n, i = 0;
  int depth = 0;
  std::vector<Node> nodes;
  std::vector<ByteSet> sets;
  std::map<std::string, int> set_ids;
  std::string err;

  int fail(const std::string& m) {
    if (err.empty()) err = m;
    return -1;
  }
  int add(Node nd) {
    nodes.push_back(std::move(nd));
    return (int)nodes.size() - 1;
  }
  int add_set(const ByteSet& s) {
    const std::string key = s.to_string();
    auto it = set_ids.find(key);
    if (it == set_ids.end()) {
      sets.push_back(s);
      it = set_ids.emplace(key, (int)sets.size() - 1).first;
    }
    Node nd;
    nd.kind = Node::SET;
    nd.set = it->second;
    return add(std::move(nd));
  }
  static std::string show(int c) {
    char b[16];
    if (c >= 0x20 && c < 0x7F) snprintf(b, sizeof b, "'%c'", c);
    else snprintf(b, sizeof b, "0x%02X", c);
    return b;
  }

  int parse_alt() {
    std::vector<int> alts;
    for (;;) {
      const int a = parse_cat();
      if (a < 0) return -1;
      alts.push_back(a);
      if (i < n && p[i] == '|') { ++i; continue; }
      break;
    }
    if (alts.size() == 1) return alts[0];
    Node nd;
    nd.kind = Node::ALT;
    nd.kids = std::move(alts);
    return add(std::move(nd));
  }

  int parse_cat() {
    std::vector<int> items;
    while (i < n && p[i] != '|' && p[i] != ')') {
      const int a = parse_repeat();
      if (a < 0) return -1;
      items.push_back(a);
    }
    if (items.size() == 1) return items[0];
    Node nd;
    nd.kind = items.empty() ? Node::EMPTY : Node::CAT;
    nd.kids = std::move(items);
    return add(std::move(nd));
  }

  // digits of a repeat bound; -1 when there are none, -2 (with the error set) past kRegexMaxRepeat
  int parse_bound() {
    if (i >= n || !is_digit(p[i])) return -1;
    int v = 0;
    while (i < n && is_digit(p[i])) {
      v = v * 10 + (p[i++] - '0');
      if (v > kRegexMaxRepeat) { fail("a repeat bound above " + std::to_string(kRegexMaxRepeat)); return -2; }
    }
    return v;
  }

  int parse_repeat() {
    const int a = parse_atom();
    if (a < 0 || i >= n) return a;
    const int c = p[i];
    if (c != '*' && c != '+' && c != '?' && c != '{') return a;
    if (nodes[a].kind == Node::BOL || nodes[a].kind == Node::EOL) return fail("a quantifier applied to ^ or $");
    int lo = 0, hi = -1;
    ++i;
    if (c == '+') lo = 1;
    else if (c == '?') hi = 1;
    else if (c == '{') {
      if (i < n && p[i] == ',') return fail("a {,n} quantifier");
      lo = parse_bound();
      if (lo == -2) return -1;
      if (lo < 0) return fail("a '{' that does not open a well-formed quantifier");
      if (i < n && p[i] == '}') { ++i; hi = lo; }
      else if (i < n && p[i] == ',') {
        ++i;
        if (i < n && p[i] == '}') { ++i; hi = -1; }
        else {
          hi = parse_bound();
          if (hi == -2) return -1;
          if (hi < 0 || i >= n || p[i] != '}') return fail("a '{' that does not open a well-formed quantifier");
          ++i;
          if (hi < lo) return fail("a {n,m} quantifier with n > m");
        }
      } else return fail("a '{' that does not open a well-formed quantifier");
    }
    if (i < n) {
      if (p[i] == '?') return fail("a lazy quantifier");
      if (p[i] == '+') return fail("a possessive quantifier");
      if (p[i] == '*' || p[i] == '{') return fail("a quantifier with nothing to repeat (it follows a quantifier)");
    }
    Node nd;
    nd.kind = Node::REP;
    nd.lo = lo;
    nd.hi = hi;
    nd.kids.push_back(a);
    return add(std::move(nd));
  }

  int parse_atom() {
    const int c = p[i];
    if (c >= 0x80) return fail("a non-ASCII byte in the pattern");
    switch (c) {
      case '(': {
        ++i;
        if (i < n && p[i] == '?') {
          if (i + 1 < n && p[i + 1] == ':') i += 2;
          else return fail("a '(?' group other than '(?:'");
        }
        if (++depth > kMaxDepth) return fail("groups nested deeper than " + std::to_string(kMaxDepth));
        const int a = parse_alt();
        --depth;
        if (a < 0) return -1;
        if (i >= n || p[i] != ')') return fail("unbalanced parentheses");
        ++i;
        Node nd;  // a node of its own: a group may be repeated even where it holds only an anchor
        nd.kind = Node::CAT;
        nd.kids.push_back(a);
        return add(std::move(nd));
      }
      case '*': case '+': case '?': return fail("a quantifier with nothing to repeat");
      case '{': return fail("a '{' that does not open a well-formed quantifier");
      case ']': case '}': return fail(std::string("an unescaped ") + show(c) + " outside its construct");
      case '[': return parse_class();
      case '.': { ++i; ByteSet s; s.set(); return add_set(s); }
      case '^': { ++i; Node nd; nd.kind = Node::BOL; return add(std::move(nd)); }
      case '$': { ++i; Node nd; nd.kind = Node::EOL; return add(std::move(nd)); }
      case '\\': {
        if (i + 1 >= n) return fail("a trailing backslash");
        const int e = p[i + 1];
        if (e >= 0x80) return fail("a non-ASCII byte in the pattern");
        i += 2;
        ByteSet s;
        if (!is_alnum(e)) { s[e] = true; return add_set(s); }
        if (e == 't') { s['\t'] = true; return add_set(s); }
        if (shorthand(e, &s)) return add_set(s);
        return fail(std::string("the escape \\") + (char)e);
      }
      default: {
        ++i;
        ByteSet s;
        s[c] = true;
        fold_case(s);
        return add_set(s);
      }
    }
  }

  int parse_class() {
    ++i;  // '['
    bool negate = false;
    if (i < n && p[i] == '^') { negate = true; ++i; }
    if (i < n && p[i] == ']') return fail("a character class that begins with ']'");
    ByteSet s;
    bool first = true;
    for (;; first = false) {
      if (i >= n) return fail("unbalanced brackets");
      const int c = p[i];
      if (c >= 0x80) return fail("a non-ASCII byte in the pattern");
      if (c == ']') { ++i; break; }
      if (c == '[') return fail("a '[' inside a character class");
      if (c == '&' && i + 1 < n && p[i + 1] == '&') return fail("'&&' inside a character class");
      if (c == '\\') {
        if (i + 1 >= n) return fail("a trailing backslash");
        const int e = p[i + 1];
        if (e >= 0x80) return fail("a non-ASCII byte in the pattern");
        ByteSet sh;
        if (!is_alnum(e)) s[e] = true;
        else if (shorthand(e, &sh)) s |= sh;
        else return fail(std::string("the escape \\") + (char)e + " inside a character class");
        i += 2;
        continue;
      }
      if (c == '-') {  // a literal only when first or last (a range's '-' is consumed with its left end below)
        if (first || (i + 1 < n && p[i + 1] == ']')) { s['-'] = true; ++i; continue; }
        return fail("a '-' inside a character class that is neither first, last, escaped nor between the ends of a range");
      }
      if (i + 2 < n && p[i + 1] == '-' && p[i + 2] != ']') {  // a range c-d
        const int d = p[i + 2];
        const bool same = (is_digit(c) && is_digit(d)) || (is_lower(c) && is_lower(d)) || (is_upper(c) && is_upper(d));
        if (!same || d < c)
          return fail(std::string("the character class range ") + show(c) + "-" + show(d) +
                      " (both ends must be digits, lower-case or upper-case letters, in order)");
        for (int b = c; b <= d; ++b) s[b] = true;
        i += 3;
        continue;
      }
      s[c] = true;  // (a '^' that is not first is a literal)
      ++i;
    }
    fold_case(s);
    if (negate) s = ~s;
    return add_set(s);
  }
};

struct NState {
  enum Type { SPLIT, SET, BOL, EOL, ACCEPT } type = SPLIT;
  int set = -1;
  int out1 = -1, out2 = -1;
};

struct Nfa {
  std::vector<NState> st;
  bool overflow = false;
  int add(NState::Type t, int set, int o1, int o2) {
    if ((int)st.size() >= kMaxNfaStates) { overflow = true; return 0; }
    NState s;
    s.type = t;
    s.set = set;
    s.out1 = o1;
    s.out2 = o2;
    st.push_back(s);
    return (int)st.size() - 1;
  }
};

// The states of `node` in front of state `next`; returns the entry.
int emit(const std::vector<Node>& nodes, int node, int next, Nfa& nfa) {
  if (nfa.overflow) return next;
  const Node& nd = nodes[node];
  switch (nd.kind) {
    case Node::EMPTY: return next;
    case Node::SET: return nfa.add(NState::SET, nd.set, next, -1);
    case Node::BOL: return nfa.add(NState::BOL, -1, next, -1);
    case Node::EOL: return nfa.add(NState::EOL, -1, next, -1);
    case Node::CAT: {
      int cur = next;
      for (size_t k = nd.kids.size(); k-- > 0;) cur = emit(nodes, nd.kids[k], cur, nfa);
      return cur;
    }
    case Node::ALT: {
      int cur = emit(nodes, nd.kids.back(), next, nfa);
      for (size_t k = nd.kids.size() - 1; k-- > 0;) cur = nfa.add(NState::SPLIT, -1, emit(nodes, nd.kids[k], next, nfa), cur);
      return cur;
    }
    default: {  // REP
      const int kid = nd.kids[0];
      int cur = next;
      if (nd.hi < 0) {  // x{lo,}: lo copies in front of a loop
        const int loop = nfa.add(NState::SPLIT, -1, -1, next);
        const int body = emit(nodes, kid, loop, nfa);
        if (!nfa.overflow) nfa.st[loop].out1 = body;
        cur = loop;
      } else {  // x{lo,hi}: hi - lo nested optional copies
        for (int k = nd.lo; k < nd.hi && !nfa.overflow; ++k) cur = nfa.add(NState::SPLIT, -1, emit(nodes, kid, cur, nfa), next);
      }
      for (int k = 0; k < nd.lo && !nfa.overflow; ++k) cur = emit(nodes, kid, cur, nfa);
      return cur;
    }
  }
}

struct Builder {
  const Nfa& nfa;
  const std::vector<ByteSet>& sets;
  std::vector<uint32_t> stamp;
  uint32_t tick = 0;
  std::vector<int> stack;
  int64_t work = 0;

  Builder(const Nfa& a, const std::vector<ByteSet>& s) : nfa(a), sets(s), stamp(a.st.size(), 0) {}

  // The states reachable from `seeds` without input, `^` edges taken when bol and `$` edges when eol, as the sorted
  // list of those that can still act (SET, EOL, ACCEPT); *accepts when the accepting state is among them.
  void closure(const std::vector<int>& seeds, bool bol, bool eol, std::vector<int>* out, bool* accepts) {
    ++tick;
    out->clear();
    *accepts = false;
    stack.assign(seeds.begin(), seeds.end());
    while (!stack.empty()) {
      const int s = stack.back();
      stack.pop_back();
      if (s < 0 || stamp[s] == tick) continue;
      stamp[s] = tick;
      ++work;
      const NState& ns = nfa.st[s];
      switch (ns.type) {
        case NState::SPLIT: stack.push_back(ns.out1); stack.push_back(ns.out2); break;
        case NState::BOL: if (bol) stack.push_back(ns.out1); break;
        case NState::EOL:
          if (eol) stack.push_back(ns.out1);
          else out->push_back(s);
          break;
        case NState::SET: out->push_back(s); break;
        case NState::ACCEPT: *accepts = true; out->push_back(s); break;
      }
    }
    std::sort(out->begin(), out->end());
  }
};

}  // namespace

int regex_compile(const char* pattern, size_t len, RegexDfa* out, std::string* err) {
  auto decline = [&](const std::string& m) {
    if (err) *err = m;
    return 1;
  };
  if (len > (size_t)kRegexMaxPattern)
    return decline("a pattern longer than " + std::to_string(kRegexMaxPattern) + " bytes");
  Parser ps;
  ps.p = reinterpret_cast<const uint8_t*>(pattern);
  ps.n = len;
  const int root = ps.parse_alt();
  if (root < 0) return decline(ps.err);
  if (ps.i < len) return decline("unbalanced parentheses");  // a ')' nobody opened

  Nfa nfa;
  const int accept = nfa.add(NState::ACCEPT, -1, -1, -1);
  const int start = emit(ps.nodes, root, accept, nfa);
  if (nfa.overflow)
    return decline("a pattern whose repeats unroll into more than " + std::to_string(kMaxNfaStates) + " NFA states");

  // byte classes: bytes that every set of the pattern treats alike; EOS is a class of its own
  RegexDfa d;
  int ncls = 0;
  {
    std::map<std::vector<bool>, int> ids;
    for (int b = 0; b < 256; ++b) {
      std::vector<bool> sig(ps.sets.size());
      for (size_t k = 0; k < ps.sets.size(); ++k) sig[k] = ps.sets[k][b];
      auto it = ids.find(sig);
      if (it == ids.end()) it = ids.emplace(std::move(sig), ncls++).first;
      d.cls[b] = (uint8_t)it->second;
    }
    d.cls[kRegexEos] = (uint8_t)ncls++;
  }
  std::vector<int> rep(ncls - 1, 0);  // a byte of each class
  for (int b = 255; b >= 0; --b) rep[d.cls[b]] = b;

  // subset construction.  DFA state 0 accepts (absorbing); the others are sets of NFA states, the start state marked
  // with the pseudo state `at_begin` (only there may a `^` behind a `$` still hold, at EOS of the empty value).
  Builder B(nfa, ps.sets);
  const int at_begin = (int)nfa.st.size();
  std::map<std::vector<int>, int> ids;
  std::vector<std::vector<int>> states(1);
  std::vector<int> next_of;  // [state * ncls + class], state ids
  auto too_large = [&](size_t nstates) { return (int64_t)nstates * ncls * 2 > kRegexMaxTableBytes; };
  bool over = false;
  auto intern = [&](std::vector<int>& set, bool accepts) -> int {
    if (accepts) return 0;
    auto it = ids.find(set);
    if (it != ids.end()) return it->second;
    if (too_large(states.size() + 1)) { over = true; return 0; }
    const int id = (int)states.size();
    ids.emplace(set, id);
    states.push_back(set);
    return id;
  };
  std::vector<int> seeds, set;
  bool acc = false;
  if (too_large(1)) over = true;
  seeds.assign(1, start);
  B.closure(seeds, true, false, &set, &acc);
  set.push_back(at_begin);
  const int dstart = over ? 0 : intern(set, acc);
  next_of.assign(ncls, 0);  // row 0: absorbing
  for (size_t s = 1; s < states.size() && !over; ++s) {
    next_of.resize((s + 1) * ncls, 0);
    const std::vector<int> cur = states[s];
    const bool begin = !cur.empty() && cur.back() == at_begin;
    for (int c = 0; c < ncls - 1 && !over; ++c) {
      seeds.assign(1, start);  // the search prefix: a match may begin at every position
      for (int q : cur)
        if (q != at_begin && nfa.st[q].type == NState::SET && ps.sets[nfa.st[q].set][rep[c]]) seeds.push_back(nfa.st[q].out1);
      B.closure(seeds, false, false, &set, &acc);
      next_of[s * ncls + c] = intern(set, acc);
    }
    seeds.clear();
    for (int q : cur)
      if (q != at_begin) seeds.push_back(q);
    B.closure(seeds, begin, true, &set, &acc);
    next_of[s * ncls + ncls - 1] = acc ? 0 : (int)s;  // nothing is read after EOS
    if (B.work > kMaxWork) return decline("a pattern whose automaton takes too long to build");
  }
  if (over)
    return decline("a DFA transition table above PGPU_REGEX_MAX_TABLE_BYTES (" + std::to_string(kRegexMaxTableBytes) +
                   " bytes: more than " + std::to_string(states.size()) + " states x " + std::to_string(ncls) +
                   " byte classes x 2)");
  d.num_states = (int32_t)states.size();
  d.num_classes = ncls;
  d.table.resize(next_of.size());
  for (size_t k = 0; k < next_of.size(); ++k) d.table[k] = (uint16_t)(next_of[k] * ncls);
  d.start_row = (uint16_t)(dstart * ncls);
  *out = std::move(d);
  return 0;
}

bool regex_match(const RegexDfa& d, const uint8_t* value, size_t n) {
  uint32_t row = d.start_row;
  for (size_t k = 0; k < n && row != 0; ++k) row = d.table[row + d.cls[value[k]]];
  if (row == 0) return true;
  return d.table[row + d.cls[kRegexEos]] == 0;
}

}  // namespace pgpu
