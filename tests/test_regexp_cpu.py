"""REGEXP_LIKE / LIKE on the host: the LIKE conversion, the accepted subset and every declined shape, the host
interpreter of the DFA against the Python yardstick (tests/regexp_common.py), the parser, and the stand-alone
sanitizer program over the pattern compiler."""
import json
import os
import random
import subprocess

import pytest

import regexp_common as rc
from pinot_amd import _lib as L
from pinot_amd.query import (FilterContext, Predicate, REGEXP_LIKE, check_regexp_pattern, like_to_regexp_like,
                             parse_query)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_like_to_regexp.json")


# ------------------------------------------------------------------------------------------------ LIKE conversion
def test_like_conversion_known_answers():
    with open(GOLDEN) as f:
        pairs = json.load(f)["pairs"]
    assert len(pairs) == 8
    for p in pairs:
        assert like_to_regexp_like(p["like"]) == p["regexp"], p


def test_like_conversion_every_metacharacter():
    # the 19 metacharacters in the reference's order, then both wildcards and plain text
    like = "\\^$.{}[]()*+?|<>-&/" + "_%ab"
    assert len(set(like[:19])) == 19
    want = "^" + "".join("\\" + c for c in like[:19]) + "..*ab" + "$"
    assert like_to_regexp_like(like) == want
    # the backslash is escaped first, so the escapes added for the other characters are not escaped again
    assert like_to_regexp_like("\\.") == "^\\\\\\.$"
    assert like_to_regexp_like("") == "^$"
    # every converted pattern is inside the accepted subset
    L.regex_check(want)


# ------------------------------------------------------------------------------------------------ the subset
ACCEPTED = [
    "", "abc", "aBc", ".", "a.c", "^a", "a$", "^$", "a^b", "$^", "(^a|b$)", "(a)", "(?:a)", "(a|b)", "(a|)", "(|a)", "()",
    "a|b|c", "a|", "a*", "a+", "a?", "a{2}", "a{2,}", "a{2,3}", "a{0}", "a{64}", "(ab){2,3}$", "(a|b)*abb", "(^)*a",
    "[abc]", "[^abc]", "[a-c]", "[A-C]", "[0-9]", "[a-cX-Z0-3_]", "[-a]", "[a-]", "[^-a]", "[a\\-z]", "[a^]", "[\\^a]",
    "[\\d-]", "[\\w.]", "[\\s]", "[\\D]", "[^\\W]", "[\\S\\d]", "[\\]\\[]", "[&]", "[a&b]", "[.*+?(){}|$]",
    "\\.", "\\\\", "\\<\\>\\-\\&\\/", "\\^\\$", "\\{\\}\\[\\]\\(\\)\\*\\+\\?\\|", "\\t", "\\ ", "\\_", "\\d+", "\\D", "\\w*",
    "\\W", "\\s", "\\S", "a b", "x" * 1024, "^.*\\.html$", "(a{2}){3}", "(a*)*", "((((a))))+",
]

DECLINED = [
    ("\\1", "\\1"), ("(a)\\1", "\\1"), ("\\b", "\\b"), ("\\B", "\\B"), ("\\A", "\\A"), ("\\z", "\\z"), ("\\Z", "\\Z"),
    ("\\G", "\\G"), ("\\Qa\\E", "\\Q"), ("\\E", "\\E"), ("\\p{L}", "\\p"), ("\\P{L}", "\\P"), ("\\x41", "\\x"),
    ("\\u0041", "\\u"), ("\\0101", "\\0"), ("\\cA", "\\c"), ("\\h", "\\h"), ("\\v", "\\v"), ("\\R", "\\R"),
    ("\\k<n>", "\\k"), ("\\n", "\\n"), ("\\r", "\\r"), ("\\f", "\\f"), ("\\a", "\\a"), ("\\e", "\\e"),
    ("(?i)a", "(?"), ("(?=a)", "(?"), ("(?!a)", "(?"), ("(?<n>a)", "(?"), ("(?<=a)b", "(?"), ("(?>a)", "(?"),
    ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{2}?", "lazy"), ("a*+", "possessive"), ("a++", "possessive"),
    ("a?+", "possessive"), ("a{2,3}+", "possessive"),
    ("*a", "nothing to repeat"), ("+", "nothing to repeat"), ("?", "nothing to repeat"), ("a|*", "nothing to repeat"),
    ("(*a)", "nothing to repeat"), ("a**", "nothing to repeat"), ("a{2}{3}", "nothing to repeat"),
    ("^*", "^ or $"), ("$+", "^ or $"), ("^{2}", "^ or $"), ("a$?", "^ or $"),
    ("a{,3}", "{,n}"), ("a{", "'{'"), ("a{x}", "'{'"), ("a{2", "'{'"), ("a{2,x}", "'{'"), ("{2}", "'{'"), ("a{3,2}", "n > m"),
    ("a{65}", "above 64"), ("a{2,65}", "above 64"), ("a{65,}", "above 64"),
    ("a]", "']'"), ("a}", "'}'"), ("]", "']'"),
    ("[a[b]]", "'['"), ("[a&&b]", "&&"), ("[]a]", "begins with ']'"), ("[]", "begins with ']'"), ("[^]a]", "begins with ']'"),
    ("[a-Z]", "range"), ("[A-z]", "range"), ("[0-a]", "range"), ("[z-a]", "range"), ("[ -~]", "range"), ("[a-\\d]", "range"),
    ("[\\d-z]", "'-'"), ("[a-c-e]", "'-'"), ("[\\t]", "\\t"), ("[\\b]", "\\b"),
    ("\u00e9", "non-ASCII"), ("[\u00e9]", "non-ASCII"), ("\\\u00e9", "non-ASCII"),
    ("a\\", "trailing backslash"), ("[a\\", "trailing backslash"),
    ("(a", "parentheses"), ("a)", "parentheses"), ("((a)", "parentheses"), ("[a", "brackets"), ("[^", "brackets"),
    ("x" * 1025, "longer than 1024"),
    ("(a|b)*a(a|b){12}", "PGPU_REGEX_MAX_TABLE_BYTES"),
]


@pytest.mark.parametrize("pattern", ACCEPTED)
def test_accepted_by_both_layers(pattern):
    states, classes, table_bytes = L.regex_check(pattern)
    assert states >= 1 and classes >= 2 and 0 < table_bytes == states * classes * 2 <= L.REGEX_MAX_TABLE_BYTES
    assert check_regexp_pattern(pattern) == (states, classes, table_bytes)
    p = Predicate.regexp_like("c", pattern)
    assert (p.type, p.column, p.values) == (REGEXP_LIKE, "c", [pattern])


@pytest.mark.parametrize("pattern,word", DECLINED)
def test_declined_by_both_layers(pattern, word):
    with pytest.raises(L.UnsupportedQueryError) as e:
        L.regex_check(pattern.encode("utf-8"))
    assert e.value.code == L.PGPU_ERR_UNSUPPORTED
    assert "REGEXP_LIKE" in e.value.message and word in e.value.message, e.value.message
    with pytest.raises(ValueError) as v:
        Predicate.regexp_like("c", pattern)
    assert "REGEXP_LIKE" in str(v.value)


def test_table_cap_message():
    with pytest.raises(L.UnsupportedQueryError) as e:
        L.regex_check("(a|b)*a(a|b){12}")
    assert "PGPU_REGEX_MAX_TABLE_BYTES" in e.value.message and "32768" in e.value.message
    # one repeat fewer halves the states and fits: the cap is a table size, not a pattern shape
    states, classes, table_bytes = L.regex_check("(a|b)*a(a|b){11}")
    assert states > 2048 and L.REGEX_MAX_TABLE_BYTES // 2 < table_bytes <= L.REGEX_MAX_TABLE_BYTES


# ------------------------------------------------------------------------------------------------ the host DFA
VALUES = ["", "a", "A", "b", "ab", "AB", "ba", "aa", "caa", "caaa", "aaaa", "ca", "abc", "aBc", "xabcx", "_", "-", "5", "a5",
          "a b", "a\tb", " ", ".", "a.c", "abb", "babb", "z", "Z", "q", "^", "$", "a^b", "a$", "[", "]", "\\", "a|b", "<>-&/",
          "x.html", "x.htmlx", "foo/bar.html", "{}", "()", "*+?", "0", "9", "a-z", "&", "~"]


@pytest.mark.parametrize("pattern", [p for p in ACCEPTED if len(p) < 100])
def test_host_dfa_matches_yardstick_fixed(pattern):
    for v in VALUES:
        assert L.regex_match_host(pattern, v) == rc.yardstick(pattern, v), (pattern, v)


def test_host_dfa_named_cases():
    cases = [("", "", True), ("", "abc", True), ("^$", "", True), ("^$", "a", False), ("a^b", "ab", False), ("a^b", "a^b", False),
             ("(^a|b$)", "ab", True), ("(^a|b$)", "ba", False), ("(^a|b$)", "xb", True), ("[^a]", "A", False),
             ("[^a]", "b", True), ("\\W", "_", False), ("\\W", "-", True), ("[\\d-]", "-", True), ("[\\d-]", "7", True),
             ("[\\d-]", "d", False), ("a{2,3}$", "caa", True), ("a{2,3}$", "ca", False), ("a{2,3}$", "aaaa", True),
             ("a{2,3}$", "aab", False), ("abc", "xABCx", True), ("[abc]x", "Bx", True), ("[a-c]x", "CX", True),
             ("[A-C]x", "bx", True), ("[^a-c]", "B", False), ("$^", "", True), ("$^", "a", False), ("^^a", "a", True)]
    for pattern, value, want in cases:
        assert rc.yardstick(pattern, value) == want, (pattern, value)
        assert L.regex_match_host(pattern, value) == want, (pattern, value)


def test_host_dfa_fuzz_against_yardstick():
    patterns = rc.random_patterns(20260, 2000)
    values = rc.random_values(977, 50)
    declined, bad, matches = [], [], 0
    for p in patterns:
        try:
            L.regex_check(p)
        except L.UnsupportedQueryError as e:
            assert "PGPU_REGEX_MAX_TABLE_BYTES" in e.message, (p, e.message)  # the only decline a subset pattern may meet
            declined.append(p)
            continue
        for v in values:
            want = rc.yardstick(p, v)
            matches += want
            if L.regex_match_host(p, v) != want:
                bad.append((p, v, want))
    assert not bad, bad[:10]
    assert len(declined) <= len(patterns) // 10, len(declined)
    # the generators are no strawmen: both outcomes are common
    assert len(patterns) * len(values) // 10 < matches < len(patterns) * len(values) * 9 // 10


def test_generators_are_seeded():
    assert rc.random_patterns(5, 20) == rc.random_patterns(5, 20) != rc.random_patterns(6, 20)
    assert rc.random_values(5, 20) == rc.random_values(5, 20)
    rng = random.Random(1)
    for _ in range(200):
        p = rc.random_pattern(rng)
        rc.yardstick(p, "")  # Python reads every generated pattern


# ------------------------------------------------------------------------------------------------ the parser
def _where(text, **kw):
    return parse_query("SELECT COUNT(*) FROM t WHERE %s GROUP BY g" % text, **kw).filter


def test_parse_round_trips():
    f = _where("url LIKE 'foo%'")
    assert f.type == FilterContext.PREDICATE
    assert (f.predicate.type, f.predicate.column, f.predicate.values) == (REGEXP_LIKE, "url", ["^foo.*$"])
    f = _where("url NOT LIKE '%.html'")
    assert f.type == FilterContext.NOT and f.children[0].predicate.values == ["^.*\\.html$"]
    f = _where("REGEXP_LIKE(url, '^/a/[0-9]+$')")
    assert (f.predicate.type, f.predicate.column, f.predicate.values) == (REGEXP_LIKE, "url", ["^/a/[0-9]+$"])
    f = _where("NOT REGEXP_LIKE(url, 'x')")
    assert f.type == FilterContext.NOT and f.children[0].predicate.values == ["x"]
    f = _where("regexp_like(url, 'it''s')")  # the keyword in any case; a doubled quote is one quote
    assert f.predicate.values == ["it's"]
    f = _where("a LIKE 'x_' AND (NOT REGEXP_LIKE(b, 'y') OR c NOT LIKE 'z') AND d > 3")
    assert f.type == FilterContext.AND and [k.type for k in f.children] == ["PREDICATE", "OR", "PREDICATE"]
    preds, ops = [], []
    f.postfix(preds, ops)
    assert [(p.type, p.column, p.values) for p in preds] == [
        (REGEXP_LIKE, "a", ["^x.$"]), (REGEXP_LIKE, "b", ["y"]), (REGEXP_LIKE, "c", ["^z$"]), ("RANGE", "d", ["3", "*"])]
    assert ops == [(L.OP_PRED, 0), (L.OP_PRED, 1), (L.OP_NOT, 0), (L.OP_PRED, 2), (L.OP_NOT, 0), (L.OP_OR, 2), (L.OP_PRED, 3),
                   (L.OP_AND, 3)]
    # the same under the flags GpuTable parses its SQL with
    f = _where("url LIKE 'a%' OR x * 2 > 3", filter_expressions=True, group_by_expressions=True)
    assert f.children[0].predicate.type == REGEXP_LIKE and f.children[1].predicate.column == "mult(x,2.0)"
    q = parse_query("SELECT COUNT(*) FROM t WHERE url LIKE 'a%' GROUP BY g")
    assert q.columns() == ["url", "g"]
    # columns may still be called like or regexp_like: only the keyword positions are read as the keywords
    assert _where("like = 1").predicate.column == "like"
    assert _where("regexp_like > 3").predicate.column == "regexp_like"
    f = _where("like LIKE 'a_' AND REGEXP_LIKE(regexp_like, 'b')")
    assert [(k.predicate.column, k.predicate.values) for k in f.children] == [("like", ["^a.$"]), ("regexp_like", ["b"])]
    assert _where("like NOT LIKE 'a'").children[0].predicate.column == "like"


@pytest.mark.parametrize("text,kw", [
    ("REGEXP_LIKE(url, '\\bfoo')", {}),   # outside the subset: before any plan
    ("REGEXP_LIKE(url, other)", {}), ("url LIKE other", {}),   # a pattern that is no literal
    ("REGEXP_LIKE(a + b, 'x')", {}), ("REGEXP_LIKE('x', 'x')", {}), ("REGEXP_LIKE(url)", {}),
    ("a + b LIKE 'x'", {}), ("a * b LIKE 'x'", {"filter_expressions": True}),
    ("a * b NOT LIKE 'x'", {"filter_expressions": True}), ("REGEXP_LIKE(a * b, 'x')", {"filter_expressions": True}),
    ("REGEXP_LIKE(url, 'caf\u00e9')", {}), ("REGEXP_LIKE(url, '(a|b)*a(a|b){12}')", {}),
    ("url LIKE", {}), ("url NOT LIKE", {}),
])
def test_parse_value_errors(text, kw):
    with pytest.raises(ValueError):
        _where(text, **kw)


# ------------------------------------------------------------------------------------------------ host sanitizers
def test_regex_fuzz_under_host_sanitizers():
    """tools/regex_fuzz.cpp with regex_dfa.cpp alone, built with AddressSanitizer + UndefinedBehaviorSanitizer and run as
    a child process of its own (nothing loaded into Python runs under a sanitizer)."""
    from pinot_amd import build
    exe = build.build_regex_fuzz()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, "6000", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stdout[-4000:]
    assert "regex_fuzz ok" in res.stdout
