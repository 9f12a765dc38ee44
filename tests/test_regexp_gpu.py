"""REGEXP_LIKE / LIKE on the GPU: the DFA kernel at its edges (pgpu_table_regexp_dict_ids against the host DFA and the
Python yardstick), the local sets behind the scan's LEAF_SET, and whole queries -- groups and the statistics tuple equal
to the oracle's for the same query with the predicate replaced by IN (the values the yardstick matches): on a plain
column the oracle's IN is the same scan leaf.  Tables of 3 segments of 20 000 docs unless said otherwise."""
import copy
import random
from dataclasses import replace

import numpy as np
import pytest

import regexp_common as rc
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import FilterContext, Predicate, REGEXP_LIKE, parse_query
from pinot_amd.segment import SegmentBuffers
from pinot_amd.segment_files import build_inverted_index

pytestmark = pytest.mark.gpu


# ================================================================================================ kernel edges
def _unique_values(seed, n):
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add(rc.random_value(rng, 10) if n > 1 else "ab")
    return sorted(out)


def _string_table(oracle, values):
    """One segment whose only column holds every value once: the global dictionary is sorted(values)."""
    schema = [("s", "STRING")]
    t = GpuTable(schema)
    t.pin_segment(oracle.make_segment(schema, {"s": list(values)}))
    return t


def _check_ids(t, values, pattern):
    vocab = t.dictionary("s")
    assert vocab == sorted(values)
    got, words = t.regexp_dict_ids("s", pattern)
    host = [L.regex_match_host(pattern, v) for v in vocab]
    want = [rc.yardstick(pattern, v) for v in vocab]
    assert host == want, pattern
    assert got.tolist() == want, (pattern, [v for v, a, b in zip(vocab, got.tolist(), want) if a != b][:5])
    # the spare bits of the last ballot word are 0
    n = len(vocab)
    assert len(words) == (n + 63) // 64
    if n % 64:
        assert int(words[-1]) >> (n % 64) == 0
    return sum(want)


def test_dictionary_device_copy_is_counted(oracle, gpu_lib):
    """pgpu_table_device_bytes grows by exactly the blob (padded to whole 8-byte words plus one) and offsets[n + 1] at the
    first use -- this reader builds no LUT --, once."""
    values = _unique_values(9, 100)
    with _string_table(oracle, values) as t:
        before = t.device_bytes()
        _check_ids(t, values, "a")
        total = sum(len(v) for v in values)
        want = ((total + 7) // 8 * 8 + 8) + 4 * (len(values) + 1)
        assert t.device_bytes() - before == want
        _check_ids(t, values, "b")
        assert t.device_bytes() - before == want


EDGE_PATTERNS = ["a", "^a", "b$", "^$", "", "[ab]{2}", "(a|b)*abb", "a.b", "\\d+[-_]", "^[^a]", "zzz", "(^|/)a", "1$|^0", "\\W"]


@pytest.mark.parametrize("card", [1, 63, 64, 65, 4097])
def test_cardinalities_around_the_ballot_word_and_the_workgroup(oracle, gpu_lib, card):
    values = _unique_values(card, card)
    with _string_table(oracle, values) as t:
        hits = [_check_ids(t, values, p) for p in EDGE_PATTERNS + rc.random_patterns(card, 6)]
        assert card < 64 or (max(hits) == card and min(hits) == 0 and any(0 < h < card for h in hits))


LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 300]


def test_value_lengths_around_every_load_width(oracle, gpu_lib):
    rng = random.Random(3)
    values = set()
    for n in LENGTHS:
        for _ in range(5):
            values.add("".join(rng.choice("abAB01_-. /") for _ in range(n)))
        if n:
            values.add("a" * (n - 1) + "z")   # matches only at its last byte
            values.add("z" + "a" * (n - 1))   # ... and only at its first
            values.add("q" * n)
    values = sorted(values)
    assert sorted({len(v) for v in values}) == LENGTHS
    with _string_table(oracle, values) as t:
        assert _check_ids(t, values, "z$") == len(LENGTHS) - 1       # only at the last byte (once per length; "z" is both)
        assert _check_ids(t, values, "^$") == 1                      # only the empty value
        assert _check_ids(t, values, "^z") == len(LENGTHS) - 1
        assert _check_ids(t, values, "^(q{60}){5}$") == 1
        assert _check_ids(t, values, "^.{8}$") >= 3
        assert _check_ids(t, values, "^.{16,17}$") >= 6
        for p in ["a", "[^a]$", "^(a|z)a*z?$", "b.*B", "", "\\s", "^[ab01_. /-]*$"] + rc.random_patterns(11, 10):
            _check_ids(t, values, p)


def test_largest_table_the_cap_admits(oracle, gpu_lib):
    letters = "abcdefghijklmnopqrstuvwxyz"
    best = None
    for n in range(560, 600):  # a literal of n bytes over 26 letters: n + 2 states x 28 classes
        lit = (letters * 30)[:n]
        try:
            tb = L.regex_check(lit)[2]
        except L.UnsupportedQueryError:
            break
        best = (lit, tb)
    lit, tb = best
    assert L.REGEX_MAX_TABLE_BYTES - 2 * 28 < tb <= L.REGEX_MAX_TABLE_BYTES  # one more state would not fit
    values = [lit, lit.upper(), "xx" + lit + "yy", lit[:-1], lit[:-1] + "A", lit[1:], lit[:200] + lit, "", "a", lit[:-1] + "!"]
    with _string_table(oracle, values) as t:
        assert _check_ids(t, values, lit) == 4


# ================================================================================================ whole queries
_ALL = sorted("/%s/p%02d.%s" % (d, i, e) for d in "abc" for i in range(10) for e in ("html", "php"))
SEG_VOCAB = [_ALL[:20],                                            # a run of the global dictionary: the affine LUT
             [v for i, v in enumerate(_ALL) if i % 3 != 0],        # strict subsets, each its own
             [v for i, v in enumerate(_ALL) if i % 4 != 1 and i >= 10]]
VOCAB = sorted(set().union(*SEG_VOCAB))                            # the table-global dictionary
assert VOCAB[:20] == SEG_VOCAB[0] and all(set(v) < set(VOCAB) for v in SEG_VOCAB)
SCHEMA = [("g", "INT"), ("n", "INT"), ("s", "STRING"), ("si", "STRING"), ("id", "INT"), ("idr", "INT"), ("k1", "INT"),
          ("k2", "INT")]
DOCS = 20000


def _columns(rng, vocab, id0):
    s = [vocab[i] for i in rng.integers(0, len(vocab), DOCS)]
    s[:len(vocab)] = vocab  # every value of the segment's vocabulary occurs
    k1, k2 = rng.integers(0, 3000, DOCS), rng.integers(0, 3000, DOCS)
    k1[:3000] = np.arange(3000)
    k2[:3000] = np.arange(3000)
    return {"g": rng.integers(0, 7, DOCS), "n": rng.integers(0, 1000, DOCS), "s": s, "si": list(s),
            "id": np.arange(id0, id0 + DOCS), "idr": np.arange(id0, id0 + DOCS)[::-1].copy(), "k1": k1, "k2": k2}


def _segment(oracle, cols):
    seg = oracle.make_segment(SCHEMA, cols)
    c = dict(seg.columns)
    ids = np.unique(np.asarray(cols["si"]), return_inverse=True)[1]
    c["si"] = replace(c["si"], inv_bytes=build_inverted_index(ids, c["si"].cardinality))
    return SegmentBuffers(seg.num_docs, c)


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(41)
    cols = [_columns(rng, v, i * DOCS) for i, v in enumerate(SEG_VOCAB)]
    segs = [_segment(oracle, c) for c in cols]
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(s) for s in segs]
    assert t.dictionary("s") == VOCAB
    yield t, hs, segs, cols
    t.close()


def _in_form(f, vocab, partial_in=None):
    """The filter with every REGEXP_LIKE predicate replaced by IN (the values of `vocab` the yardstick matches)."""
    if f.type == FilterContext.PREDICATE:
        p = f.predicate
        if p.type != REGEXP_LIKE:
            return f
        hits = [v for v in vocab if rc.yardstick(p.values[0], v)]
        for sv in partial_in or []:  # the oracle's IN must stay a scan leaf: some, not all, of every segment's values
            assert 0 < len(set(hits) & set(sv)) < len(sv), (p.values[0], len(set(hits) & set(sv)), len(sv))
        return FilterContext.pred(Predicate.in_(p.column, hits))
    return FilterContext(f.type, [_in_form(k, vocab, partial_in) for k in f.children])


def _oracle_answer(oracle, segs, q, vocab=VOCAB, seg_vocab=SEG_VOCAB):
    oq = copy.copy(q)
    oq.filter = _in_form(q.filter, vocab, seg_vocab)
    return oracle.run_groupby(SCHEMA, segs, oq)


def _run(t, hs, q, path=None, kinds=None):
    with t.plan(hs, q) as p:
        st = p.regexp_stats()  # every REGEXP_LIKE leaf of every segment is a device-built set; segment 0's LUT is affine
        leaves = sum(x.type == REGEXP_LIKE for x in _preds(q))
        assert st["sets"] == leaves * len(hs) and st["affine"] == leaves and (st["dict_bytes"] > 0) == (leaves > 0)
        if path:
            assert p.group_path() == path
        p.execute()
        r = p.finalize()
        if kinds is not None:
            assert p.leaf_kinds() == kinds
    return r


def _preds(q):
    preds = []
    if q.filter is not None:
        q.filter.postfix(preds, [])
    return preds


def _q(where, select="COUNT(*), SUM(n), MAX(n)", group_by="g", **kw):
    return parse_query("SELECT %s FROM t WHERE %s GROUP BY %s" % (select, where, group_by), **kw)


WHERES = [
    "s LIKE '%.html'",
    "s NOT LIKE '%.html'",
    "s LIKE '/_/p_3.%'",
    "REGEXP_LIKE(s, 'p0[0-4]')",
    "NOT REGEXP_LIKE(s, 'P0[0-4]\\.PHP$')",
    "REGEXP_LIKE(s, '^/[a-c]/p\\d[2-5]\\.(html|php)$')",
    "s LIKE '%p_7%' AND n < 500",
    "n >= 250 AND REGEXP_LIKE(s, '[13579]\\.')",
    "s NOT LIKE '%php' OR n BETWEEN 100 AND 200",
    "NOT (REGEXP_LIKE(s, 'p[0-9]1') OR n > 900)",
    "REGEXP_LIKE(s, 'html$') AND s LIKE '/_/p_2%' AND n > 10",
    "(s LIKE '%3.p%' OR REGEXP_LIKE(s, '5\\.h')) AND NOT n IN (1, 2, 3)",
]


@pytest.mark.parametrize("where", WHERES)
def test_answers_and_statistics_equal_the_in_form(oracle, data, where):
    t, hs, segs, _ = data
    q = _q(where)
    exp = _oracle_answer(oracle, segs, q)
    assert 0 < exp.stats[0] < 3 * DOCS
    r = _run(t, hs, q)
    assert r.as_dict() == exp.groups
    assert r.stats.as_tuple() == exp.stats


def test_no_folding(oracle, data):
    t, hs, segs, _ = data
    r = _run(t, hs, _q("REGEXP_LIKE(s, 'zzz')"), kinds={"set": 3})    # matches no value: still scanned, still counted
    assert r.as_dict() == {} and r.stats.as_tuple()[:2] == (0, 3 * DOCS)
    everything = oracle.run_groupby(SCHEMA, segs, parse_query("SELECT COUNT(*), SUM(n), MAX(n) FROM t GROUP BY g"))
    for where in ("s LIKE '/%'", "REGEXP_LIKE(s, '')"):                # matches every value: no match-all either
        r = _run(t, hs, _q(where), kinds={"set": 3})
        assert r.as_dict() == everything.groups
        assert r.stats.as_tuple()[:2] == (3 * DOCS, 3 * DOCS) and r.stats.num_total_docs == 3 * DOCS


def test_index_blind(oracle, data):
    t, hs, segs, _ = data
    for where in ("%s LIKE '%%.html'", "REGEXP_LIKE(%s, 'p0[0-4]') AND n < 500", "NOT REGEXP_LIKE(%s, '7')"):
        plain = _run(t, hs, _q(where % "s"))
        n_leaves = 2 if "AND" in where else 1
        want_kinds = {"set": 3} if n_leaves == 1 else {"set": 3, "range": 3}
        inv = _run(t, hs, _q(where % "si"), kinds=want_kinds)          # SET: neither BITMAP nor BITDIR
        assert inv.as_dict() == plain.as_dict() and inv.stats.as_tuple() == plain.stats.as_tuple()
    with t.plan(hs, _q("si IN ('/a/p00.html', '/b/p03.php')")) as p:   # the control: the index is there and an IN takes it
        assert set(p.leaf_kinds()) & {"bitmap", "bitdir"}


@pytest.mark.parametrize("group_by,path", [("g", "lds"), ("id", "global"), ("id, idr", "hash"), ("k1, k2", "partitioned")])
def test_every_group_path(oracle, data, group_by, path):
    t, hs, segs, _ = data
    q = _q("s LIKE '%.html' AND n < 700", select="COUNT(*), SUM(n)", group_by=group_by, num_groups_limit=10 ** 9)
    exp = _oracle_answer(oracle, segs, q)
    r = _run(t, hs, q, path=path)
    assert r.as_dict() == exp.groups and r.stats.as_tuple() == exp.stats


def test_filter_bitmap(data):
    t, hs, _, cols = data
    q = _q("REGEXP_LIKE(s, 'p0[0-4]') AND NOT s LIKE '%.php'")
    for h, c in zip(hs, cols):
        want = np.array([rc.yardstick("p0[0-4]", v) and not rc.yardstick("^.*\\.php$", v) for v in c["s"]])
        got = np.unpackbits(t.filter_bitmap(h, q, DOCS).view(np.uint8), bitorder="little")[:DOCS].astype(bool)
        assert 0 < want.sum() < DOCS and (got == want).all()


def test_plan_cache(oracle, data):
    t, hs, segs, _ = data
    q1, q2 = _q("REGEXP_LIKE(s, 'p0[0-3]')"), _q("REGEXP_LIKE(s, 'p0[0-4]')")  # one character apart
    e1, e2 = _oracle_answer(oracle, segs, q1), _oracle_answer(oracle, segs, q2)
    assert e1.groups != e2.groups
    for _ in range(2):  # the repeat is served by the cached plan
        r1 = _run(t, hs, _q("REGEXP_LIKE(s, 'p0[0-3]')"))
        assert r1.as_dict() == e1.groups and r1.stats.as_tuple() == e1.stats
        r2 = _run(t, hs, _q("REGEXP_LIKE(s, 'p0[0-4]')"))
        assert r2.as_dict() == e2.groups and r2.stats.as_tuple() == e2.stats


def test_segment_pinned_after_a_plan_brings_new_values(oracle, gpu_lib):
    """The old plan keeps the sets (and segments) it was planned with; a new plan sees the new snapshot, whose new values
    shift the global dictIds of the old ones."""
    rng = np.random.default_rng(43)
    cols = [_columns(rng, v, i * DOCS) for i, v in enumerate(SEG_VOCAB)]
    segs = [_segment(oracle, c) for c in cols]
    new_vocab = ["/0/p00.html", "/a/p00.htm", "/b/p05.phpx", "/d/p03.html", "/d/p04.php"] + VOCAB[25:40]
    cols4 = _columns(rng, sorted(new_vocab), 3 * DOCS)
    with GpuTable(SCHEMA) as t:
        hs = [t.pin_segment(s) for s in segs]
        q = _q("s LIKE '%.html' AND n < 800")
        old = t.plan(hs, q)
        assert old.regexp_stats()["affine"] == 1  # segment 0's dictionary is a run of the global one
        try:
            seg4 = _segment(oracle, cols4)
            h4 = t.pin_segment(seg4)
            assert t.dictionary("s") == sorted(set(VOCAB) | set(new_vocab))
            old.execute()
            r = old.finalize()
            exp = _oracle_answer(oracle, segs, q)
            assert r.as_dict() == exp.groups and r.stats.as_tuple() == exp.stats
        finally:
            old.close()
        vocab4 = sorted(set(VOCAB) | set(new_vocab))
        exp4 = _oracle_answer(oracle, segs + [seg4], q, vocab4, SEG_VOCAB + [sorted(new_vocab)])
        r4 = _run(t, hs + [h4], q, kinds={"set": 4, "range": 4})
        assert r4.as_dict() == exp4.groups and r4.stats.as_tuple() == exp4.stats
        got, _ = t.regexp_dict_ids("s", "^.*\\.html$")
        assert got.tolist() == [v.endswith(".html") for v in vocab4]


# ================================================================================================ declines
def _declined(t, hs, q):
    with pytest.raises(L.UnsupportedQueryError) as e:
        t.plan(hs, q)
    assert e.value.code == L.PGPU_ERR_UNSUPPORTED and "REGEXP_LIKE" in e.value.message, e.value.message
    return e.value.message


@pytest.mark.parametrize("bad", ["café", "two\nlines", "cr\rhere"])
def test_value_outside_the_limit_is_declined(oracle, gpu_lib, bad):
    schema = [("g", "INT"), ("s", "STRING")]
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, {"g": [1, 2, 3, 1], "s": ["abc", bad, "abd", "abc"]}))
        msg = _declined(t, [h], parse_query("SELECT COUNT(*) FROM t WHERE s LIKE 'ab%' GROUP BY g"))
        assert "'s'" in msg or " s:" in msg or "column s" in msg
        with pytest.raises(L.UnsupportedQueryError):
            t.regexp_dict_ids("s", "ab")
        # the table stays usable, for the predicates that need no automaton
        r = t.execute_groupby([h], parse_query("SELECT COUNT(*) FROM t WHERE s IN ('abc', 'abd') GROUP BY g"))
        assert r.as_dict() == {(1,): [2], (3,): [1]}


def test_other_declines(data):
    t, hs, _, _ = data
    def q_of(col, pattern):
        q = parse_query("SELECT COUNT(*) FROM t GROUP BY g")
        q.filter = FilterContext.pred(Predicate(REGEXP_LIKE, col, [pattern]))  # past the Python layer's own check
        return q
    assert "not a STRING" in _declined(t, hs, q_of("n", "1"))
    for pattern, word in (("\\bfoo", "\\b"), ("a*?", "lazy"), ("(a|b)*a(a|b){12}", "PGPU_REGEX_MAX_TABLE_BYTES"), ("[a-Z]", "range")):
        assert word in _declined(t, hs, q_of("s", pattern))
        with pytest.raises(L.UnsupportedQueryError):
            t.regexp_dict_ids("s", pattern)
    with pytest.raises(L.UnsupportedQueryError):
        t.regexp_dict_ids("n", "1")
    r = _run(t, hs, _q("s LIKE '/a/%' AND n < 10"))  # the table stays usable
    assert r.stats.num_docs_scanned > 0
