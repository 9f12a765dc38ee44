"""Arithmetic expressions in WHERE (WHERE price * qty > 1000), the parts that need no GPU: the parser's grammar under
parse_query(..., filter_expressions=True), hand-built predicates, and numEntriesScannedInFilter with an expression leaf
(pgpu_filter_entries_scanned, PGPU_LEAF_EXPRESSION) against a Python port of the reference's iterators -- written from
ExpressionScanDocIdIterator, SVScanDocIdIterator, AndDocIdSet / AndDocIdIterator and OrDocIdSet / OrDocIdIterator, not
from filter_stats.cpp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pinot_amd import _lib as L
from pinot_amd.query import FilterContext, Predicate, QueryContext, expr_columns, parse_query

EOF = -(1 << 31)          # Constants.EOF
MAX_DOC_PER_CALL = 10000  # DocIdSetPlanNode.MAX_DOC_PER_CALL


# ------------------------------------------------------------------------------------------------ parser
def _where(sql_filter, **kw):
    return parse_query("SELECT COUNT(*) FROM t WHERE " + sql_filter, filter_expressions=True, **kw)


def test_each_operator_form():
    cases = [("a * b > 10", ("RANGE", ["10", "*"], False, False)), ("a * b >= 10", ("RANGE", ["10", "*"], True, False)),
             ("a * b < 10", ("RANGE", ["*", "10"], False, False)), ("a * b <= 10", ("RANGE", ["*", "10"], False, True)),
             ("a * b = 10", ("EQ", ["10"], True, True)), ("a * b != 10", ("NOT_EQ", ["10"], True, True)),
             ("a * b <> -1.5", ("NOT_EQ", ["-1.5"], True, True)),
             ("a * b BETWEEN -2 AND 7.5", ("RANGE", ["-2", "7.5"], True, True)),
             ("a * b IN (1, 2.5, -3)", ("IN", ["1", "2.5", "-3"], True, True)),
             ("a * b NOT IN (0)", ("NOT_IN", ["0"], True, True))]
    for text, (ptype, values, li, ui) in cases:
        q = _where(text)
        p = q.filter.predicate
        assert (p.column, p.type, p.values) == ("mult(a,b)", ptype, values), text
        if ptype == "RANGE":
            assert (p.lower_inclusive, p.upper_inclusive) == (li, ui), text
        assert list(q.expressions) == ["mult(a,b)"] and q.expressions["mult(a,b)"] == ("mult", [("col", "a"), ("col", "b")])


def test_function_and_infix_forms_share_a_name():
    names = {_where(t).filter.predicate.column for t in
             ("(a - b) / 0.75 > 1", "DIV(SUB(a, b), 0.75) > 1", "divide(minus(a,b), 0.75) > 1", "((a - b)) / 0.75 > 1")}
    assert names == {"div(sub(a,b),0.75)"}
    q = parse_query("SELECT SUM(a * b), COUNT(*) FROM t WHERE TIMES(a, b) > 10 AND g = 3 GROUP BY g", filter_expressions=True)
    assert sorted(q.expressions) == ["mult(a,b)"]  # the aggregation and the predicate share one expression
    assert [k.predicate.column for k in q.filter.children] == ["mult(a,b)", "g"]
    assert q.columns() == ["a", "b", "g"]
    assert _where("x / y < 2 OR NOT c + 1 = 5").columns() == ["x", "y", "c"]
    assert expr_columns(_where("a*b + b*c/a >= 0").expressions["add(mult(a,b),div(mult(b,c),a))"]) == ["a", "b", "c"]


def test_parenthesised_term_is_boolean_first_then_arithmetic():
    q = _where("(a + b) * 2 > 3 AND (g = 1 OR g = 2)")
    assert q.filter.type == "AND"
    lhs, grp = q.filter.children
    assert lhs.predicate.column == "mult(add(a,b),2.0)" and lhs.predicate.values == ["3", "*"]
    assert grp.type == "OR" and [k.predicate.column for k in grp.children] == ["g", "g"]
    assert list(q.expressions) == ["mult(add(a,b),2.0)"]
    q = _where("((a + b) * 2 > 3) OR (a + b) > 1 OR ((g = 1))")
    assert [k.predicate.column for k in q.filter.children] == ["mult(add(a,b),2.0)", "add(a,b)", "g"]
    q = _where("NOT (a - 1) / b IN (2) AND (c < 3)")
    assert q.filter.children[0].type == "NOT" and q.filter.children[0].children[0].predicate.column == "div(sub(a,1.0),b)"
    # plain filters read as before
    plain = _where("g = 1 AND (f < -3 OR f BETWEEN 5 AND 9) AND s IN ('x', 'y')")
    assert plain.expressions == {} and plain.columns() == ["g", "f", "s"]


@pytest.mark.parametrize("text, word", [
    ("a + b + c + d + e > 0", "17 ops"), ("a / (b / (c / (d / (a / b)))) < 1", "stack of 6"),
    ("ADD(a, b, c, d, e) = 1", "5 columns")])
def test_limits_messages(text, word):
    with pytest.raises(ValueError) as e:
        _where(text)
    assert word in str(e.value)


@pytest.mark.parametrize("text", [
    "a * b < c", "a * b > c + 1", "a * b BETWEEN 1 AND c", "a + 1 IN (2, c)", "(a + b) * 2 = c",  # a column on the right
    "2 * 3 > 5", "3 < a", "ADD(1, 2.5) > 0", "a + MULT(2, 3) > 1",     # literal-only left-hand sides
    "FOO(a, b) > 1", "POW(a, 2) = 4",                                  # unknown functions
    "SUB(a, b, c) > 1", "-a > 1", "(a > 1) * 2 > 3", "a * b", "(a + b > 3"])
def test_value_errors(text):
    with pytest.raises(ValueError):
        _where(text)


def _predicates(q):
    preds = []
    q.filter.postfix(preds, [])
    return [(p.type, p.column, p.values, p.lower_inclusive, p.upper_inclusive) for p in preds]


@pytest.mark.parametrize("text", [
    's = "x"', 's IN ("x", "y")', 's NOT IN ("x")', "flag = true", 's <> "a b"', 's BETWEEN "a" AND "m"', "a < b",
    "g = 1 AND (s = \"x\" OR f < -3)", "NOT s = abc", "(s = \"x\")", "f >= 10 AND s IN ('q', \"r\", t)"])
def test_plain_predicates_parse_as_under_the_default_call(text):
    """What GpuTable parses (filter_expressions=True) of a filter without an expression is what the default call gives:
    after a plain column a double-quoted string or a bare word is the literal it has always been."""
    sql = "SELECT COUNT(*) FROM t WHERE " + text
    a, b = parse_query(sql), parse_query(sql, filter_expressions=True)
    assert _predicates(a) == _predicates(b) and b.expressions == {}
    assert a.filter.type == b.filter.type and a.columns() == b.columns()


def test_the_error_is_the_one_about_what_was_written():
    for text, word in (("a - 1 > 3 AND (b > 2", "expected op )"), ("(g = 1 OR g = 2", "expected op )"),
                       ("(a + b) * 2 < c", "right-hand side"), ("(a > 1) * 2 > 3", "boolean group"),
                       ("(a + b + c + d + e) * 2 > 0", "ops")):
        with pytest.raises(ValueError) as e:
            _where(text)
        assert word in str(e.value), (text, str(e.value))


def test_default_call_keeps_declining():
    for text in ("a * b > 3", "ADD(a, b) > 3", "g = 1 AND a + b < 3", "(a + b) * 2 > 3"):
        with pytest.raises(ValueError):
            parse_query("SELECT SUM(a) FROM t WHERE " + text)
    assert parse_query("SELECT SUM(a) FROM t WHERE (g = 1 OR g = 2) AND f < 3").filter.type == "AND"


def test_hand_built_predicates():
    f = FilterContext.and_(FilterContext.pred(Predicate.range("a * b", 3, "*", False, False)),
                           FilterContext.pred(Predicate.in_("TIMES(a, b)", [1, 2])),
                           FilterContext.pred(Predicate.eq("g", 4)))
    q = QueryContext(["g"], [("SUM", "a*b"), ("COUNT", "*")], f)
    assert [k.predicate.column for k in q.filter.children] == ["mult(a,b)", "mult(a,b)", "g"]
    # the caller's tree is left as it was given, and can be used again
    assert [k.predicate.column for k in f.children] == ["a * b", "TIMES(a, b)", "g"]
    assert q.filter.children[2] is f.children[2]
    assert _predicates(QueryContext([], [("COUNT", "*")], f)) == _predicates(q)
    assert list(q.expressions) == ["mult(a,b)"] and q.columns() == ["a", "b", "g"]
    with pytest.raises(KeyError):  # an expression is a column only once a table has registered it
        q.to_c({"a": 0, "b": 1, "g": 2})
    c, keep = q.to_c({"a": 0, "b": 1, "g": 2, "mult(a,b)": 3})
    assert [c.predicates[i].column for i in range(3)] == [3, 3, 2] and c.aggs[0].column == 3
    # `expressions` given says which names are expressions: every other one is a column, whatever its characters
    q = QueryContext([], [("COUNT", "*")], FilterContext.pred(Predicate.eq("a-b", 1)), expressions={})
    assert q.filter.predicate.column == "a-b" and q.columns() == ["a-b"]
    for bad in ("2 * 3", "SUB(a,b,c)", "FOO(a)"):
        with pytest.raises(ValueError):
            QueryContext([], [("COUNT", "*")], FilterContext.pred(Predicate.eq(bad, 1)))


# ------------------------------------------------------------------------------------------------ the iterators
class BitmapIt:
    """An index-based iterator (SortedDocIdIterator, BitmapDocIdIterator, RangelessBitmapDocIdIterator): a doc set."""
    index = True

    def __init__(self, mask):
        self.mask = mask
        self.docs = np.flatnonzero(mask)
        self.pos = 0

    def next(self):
        if self.pos < len(self.docs):
            self.pos += 1
            return int(self.docs[self.pos - 1])
        return EOF

    def advance(self, target):
        self.pos = max(self.pos, int(np.searchsorted(self.docs, target)))
        return self.next()


class ScanIt:
    """SVScanDocIdIterator: next() tests doc after doc from the cursor, each one an entry; advance() moves the cursor;
    applyAnd tests every doc it is handed."""
    index = False

    def __init__(self, mask):
        self.mask = mask
        self.n = len(mask)
        self.docs = np.flatnonzero(mask)
        self.next_doc = 0
        self.scanned = 0

    def next(self):
        if self.next_doc >= self.n:
            return EOF
        i = int(np.searchsorted(self.docs, self.next_doc))  # (the per-doc loop, counted in one step)
        if i == len(self.docs):
            self.scanned += self.n - self.next_doc
            self.next_doc = self.n
            return EOF
        d = int(self.docs[i])
        self.scanned += d - self.next_doc + 1
        self.next_doc = d + 1
        return d

    def advance(self, target):
        self.next_doc = target
        return self.next()

    def apply_and(self, docs_mask):
        self.scanned += int(docs_mask.sum())
        return docs_mask & self.mask


class ExprIt:
    """ExpressionScanDocIdIterator."""
    index = False

    def __init__(self, mask):
        self.mask = mask
        self.end = len(mask)
        self.block_end = 0
        self.it = None  # _docIdIterator: [matching docs of the block, position]
        self.scanned = 0

    def next(self):
        if self.it is not None and self.it[1] < len(self.it[0]):
            self.it[1] += 1
            return int(self.it[0][self.it[1] - 1])
        while self.block_end < self.end:
            start = self.block_end
            self.block_end = min(start + MAX_DOC_PER_CALL, self.end)
            self.scanned += self.block_end - start  # processProjectionBlock: numDocs of the block
            m = start + np.flatnonzero(self.mask[start:self.block_end])
            if len(m):
                self.it = [m, 1]
                return int(m[0])
        return EOF

    def advance(self, target):
        if target < self.block_end:
            self.it[1] = max(self.it[1], int(np.searchsorted(self.it[0], target)))  # advanceIfNeeded
            if self.it[1] < len(self.it[0]):
                self.it[1] += 1
                return int(self.it[0][self.it[1] - 1])
        else:
            self.block_end = target
        self.it = None
        return self.next()

    def apply_and(self, docs_mask):
        self.scanned += int(docs_mask.sum())  # one projection block after another: every doc handed in
        return docs_mask & self.mask


class AndIt:
    index = False

    def __init__(self, kids):
        self.kids = kids
        self.next_doc = 0

    def next(self):
        max_doc, max_idx, index = self.next_doc, -1, 0
        while index < len(self.kids):
            if index == max_idx:
                index += 1
                continue
            d = self.kids[index].advance(max_doc)
            if d == EOF:
                return EOF
            if d == max_doc:
                index += 1
            else:
                max_doc, max_idx, index = d, index, 0
        self.next_doc = max_doc + 1
        return max_doc

    def advance(self, target):
        self.next_doc = target
        return self.next()


class OrIt:
    index = False

    def __init__(self, kids):
        self.kids = list(kids)
        self.next_ids = [-1] * len(kids)
        self.prev = -1

    def _step(self, stale, move):
        nxt, exhausted = None, False
        for i in range(len(self.kids)):
            d = self.next_ids[i]
            if stale(d):
                d = move(self.kids[i])
                self.next_ids[i] = d
                if d == EOF:
                    exhausted = True
                    continue
            nxt = d if nxt is None else min(nxt, d)
        if exhausted:
            keep = [i for i in range(len(self.kids)) if self.next_ids[i] != EOF]
            self.kids = [self.kids[i] for i in keep]
            self.next_ids = [self.next_ids[i] for i in keep]
        if nxt is None:
            return EOF
        self.prev = nxt
        return nxt

    def next(self):
        return self._step(lambda d: d == self.prev, lambda k: k.next())

    def advance(self, target):
        return self._step(lambda d: d < target, lambda k: k.advance(target))


PRIORITY = {"sorted": 0, "bitmap": 1, "and": 3, "or": 4, "scan": 5, "expr": 10}  # FilterOperatorUtils.java:143-178


def build_iterator(node, masks, scans):
    """FilterBlockDocIdSet.iterator() of a tree ("and" | "or", [children]) / (leaf type, predicate index); the
    scan-based iterators are collected in `scans` (getNumEntriesScannedInFilter sums theirs)."""
    kind = node[0]
    if kind in ("sorted", "bitmap"):
        return BitmapIt(masks[node[1]])
    if kind in ("scan", "expr"):
        it = (ScanIt if kind == "scan" else ExprIt)(masks[node[1]])
        scans.append(it)
        return it
    kids = node[1]
    if kind == "and":  # reorderAndFilterChildOperators: a stable sort by priority
        kids = sorted(kids, key=lambda k: PRIORITY[k[0]])
    its = [build_iterator(k, masks, scans) for k in kids]
    idx = [i for i in its if i.index]
    scan = [i for i in its if isinstance(i, (ScanIt, ExprIt))]
    rest = [i for i in its if not i.index and not isinstance(i, (ScanIt, ExprIt))]
    if kind == "and":  # AndDocIdSet.iterator()
        if (idx and scan) or len(idx) > 1:
            docs = idx[0].mask.copy()
            for i in idx[1:]:
                docs &= i.mask
            for s in scan:
                docs = s.apply_and(docs)
            merged = BitmapIt(docs)
            return merged if not rest else AndIt([merged] + rest)
        return AndIt(its)
    if len(idx) > 1:  # OrDocIdSet.iterator()
        docs = idx[0].mask.copy()
        for i in idx[1:]:
            docs |= i.mask
        merged = BitmapIt(docs)
        other = [i for i in its if not i.index]
        return merged if not other else OrIt([merged] + other)
    return OrIt(its)


def model_entries(tree, masks):
    scans = []
    root = build_iterator(tree, masks, scans)
    if not root.index:  # (an index-based root: nothing is scanned whoever drains it)
        while root.next() != EOF:
            pass
    return sum(s.scanned for s in scans)


LEAF_CODE = {"scan": L.LEAF_SCAN, "sorted": L.LEAF_SORTED, "bitmap": L.LEAF_BITMAP, "expr": L.LEAF_EXPRESSION}


def postfix(tree, ops, types):
    if tree[0] in ("and", "or"):
        for k in tree[1]:
            postfix(k, ops, types)
        ops.append((L.OP_AND if tree[0] == "and" else L.OP_OR, len(tree[1])))
    else:
        ops.append((L.OP_PRED, tree[1]))
        types[tree[1]] = LEAF_CODE[tree[0]]


def lib_entries(tree, masks):
    n = len(masks[0])
    ops, types = [], {}
    postfix(tree, ops, types)
    words = [np.packbits(np.concatenate([m, np.zeros(-n % 32, dtype=bool)]), bitorder="little").view(np.uint32).copy()
             for m in masks]
    fo = (L.FilterOpC * len(ops))(*[L.FilterOpC(o, a) for o, a in ops])
    ty = (ctypes.c_int32 * len(masks))(*[types[i] for i in range(len(masks))])
    mk = (ctypes.c_void_p * len(masks))(*[w.ctypes.data for w in words])
    out = ctypes.c_int64()
    L.check(L.load().pgpu_filter_entries_scanned(fo, len(ops), ty, mk, len(masks), n, ctypes.byref(out)))
    return out.value


def random_mask(rng, n, kind):
    """A leaf's doc set: a docId range for a sorted leaf; else a density drawn from very sparse to almost full, now and
    then with a long empty stretch (so that blocks without a match occur)."""
    m = np.zeros(n, dtype=bool)
    if kind == "sorted":
        a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
        m[a:max(b, min(a + 1, n))] = True
    else:
        m = rng.random(n) < float(rng.choice([0.0005, 0.01, 0.2, 0.6, 0.97]))
        if rng.random() < 0.4 and n > 3:
            a, b = sorted(int(x) for x in rng.integers(0, n, 2))
            m[a:b] = False
    if not m.any():
        m[int(rng.integers(0, n))] = True
    return m


def leaf(kind, i):
    return (kind, i)


SHAPES = {
    "lone": leaf("expr", 0),
    "or(expr,scan)": ("or", [leaf("expr", 0), leaf("scan", 1)]),
    "and(bitmap,expr)": ("and", [leaf("bitmap", 0), leaf("expr", 1)]),
    "and(sorted,scan,expr)": ("and", [leaf("sorted", 0), leaf("scan", 1), leaf("expr", 2)]),
    "and(scan,expr)": ("and", [leaf("scan", 0), leaf("expr", 1)]),
    "and(expr,expr)": ("and", [leaf("expr", 0), leaf("expr", 1)]),
    "and(or(scan,scan),expr)": ("and", [("or", [leaf("scan", 0), leaf("scan", 1)]), leaf("expr", 2)]),
    "or(and(scan,expr),bitmap)": ("or", [("and", [leaf("scan", 0), leaf("expr", 1)]), leaf("bitmap", 2)]),
    "and(expr,scan) as written": ("and", [leaf("expr", 0), leaf("scan", 1)]),
    "and(expr,bitmap,scan) as written": ("and", [leaf("expr", 0), leaf("bitmap", 1), leaf("scan", 2)]),
}
NUM_DOCS = [1, 31, 9999, 10000, 10001, 25003]


def leaves_of(tree):
    return [tree] if tree[0] not in ("and", "or") else [l for k in tree[1] for l in leaves_of(k)]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_expression_leaf_counts_match_the_iterators(shape):
    tree = SHAPES[shape]
    rng = np.random.default_rng(sorted(SHAPES).index(shape) + 77)
    for n in NUM_DOCS:
        for _ in range(4):
            masks = [random_mask(rng, n, k) for k, _ in sorted(leaves_of(tree), key=lambda l: l[1])]
            assert lib_entries(tree, masks) == model_entries(tree, masks), (shape, n)


def test_lone_leaf_and_or_count_every_doc():
    rng = np.random.default_rng(5)
    for n in NUM_DOCS:
        m = [random_mask(rng, n, "expr"), random_mask(rng, n, "scan"), random_mask(rng, n, "expr")]
        assert lib_entries(SHAPES["lone"], m[:1]) == n
        assert lib_entries(SHAPES["or(expr,scan)"], m[:2]) == 2 * n
        assert lib_entries(("or", [leaf("expr", 0), leaf("bitmap", 1), leaf("expr", 2)]), m) == 2 * n


def test_worked_anchor():
    """One segment of 25003 docs, AND(scan, expr): the scan matches docs 12345 and 24000 only, the expression every doc.
    The scan counts 12346 + 11655 + 1002 = 25003; the expression evaluates blocks [12345, 22345) and [24000, 25003) --
    11003; 36006 in all."""
    n = 25003
    scan = np.zeros(n, dtype=bool)
    scan[[12345, 24000]] = True
    masks = [scan, np.ones(n, dtype=bool)]
    assert model_entries(SHAPES["and(scan,expr)"], masks) == 36006
    assert lib_entries(SHAPES["and(scan,expr)"], masks) == 36006
    assert lib_entries(SHAPES["and(expr,scan) as written"], masks[::-1]) == 36006


# Counts of the existing leaf types on fixed masks, as the library gave them before the expression leaf existed
# (default_rng(2024), 25003 docs, masks drawn in leaf order by random_mask).
BEFORE = [(("and", [leaf("scan", 0), leaf("scan", 1)]), 44798),
          (("and", [leaf("scan", 0), leaf("scan", 1), leaf("scan", 2)]), 25720),
          (("and", [leaf("sorted", 0), leaf("scan", 1)]), 682),
          (("and", [leaf("bitmap", 0), leaf("scan", 1), leaf("scan", 2)]), 27367),
          (("or", [leaf("scan", 0), leaf("bitmap", 1), leaf("sorted", 2)]), 25003),
          (("and", [("or", [leaf("scan", 0), leaf("scan", 1)]), leaf("scan", 2)]), 37661),
          (("or", [("and", [leaf("scan", 0), leaf("scan", 1)]), leaf("bitmap", 2)]), 25020),
          (("and", [leaf("sorted", 0), leaf("bitmap", 1)]), 0)]


def test_existing_leaf_types_count_as_before():
    rng = np.random.default_rng(2024)
    for tree, before in BEFORE:
        masks = [random_mask(rng, 25003, k) for k, _ in sorted(leaves_of(tree), key=lambda l: l[1])]
        got = lib_entries(tree, masks)
        assert got == model_entries(tree, masks), tree
        assert got == before, tree


# ------------------------------------------------------------------------------------------------ the host check
def test_expr_filter_check_runs_clean():
    """tools/expr_filter_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer: the task builder, the job list
    and the IT_EXPR replay (its own asserts; a stand-alone program, nothing loaded into Python)."""
    from pinot_amd import build
    exe = build.build_expr_filter_check()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout[-4000:]
    assert "expr_filter_check: ok" in res.stdout
