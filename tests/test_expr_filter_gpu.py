"""Arithmetic expressions in WHERE on the GPU (WHERE price * qty > 1000: the reference's ExpressionFilterOperator).  The
doc sets and the group rows are exact against numpy float64 evaluated op by op in the reference's order; the statistics
against the Python port of the reference's iterators in test_expr_filter_cpu.py (per segment: the leaf operator of each
predicate, AND children in the reference's order).  Two segments of 70 and 25003 docs: a partial last 32-doc group, a
partial last wave, and the 10000-doc blocks of ExpressionScanDocIdIterator crossed."""
from dataclasses import replace

import numpy as np
import pytest

import expr_common as E
import startree_common as SC
import test_expr_filter_cpu as M
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import FilterContext, Predicate, QueryContext, parse_query
from pinot_amd.segment import SegmentBuffers
from pinot_amd.segment_files import _sorted_pairs, build_inverted_index
from pinot_amd.startree import StarTree

pytestmark = pytest.mark.gpu

# g: the group column; srt: sorted; iv: with an inverted index; f: a plain scan column; a1 / a5 / a11: INT operands of
# 2, 20 and 2000 distinct values (1, 5 and 11 bits); vl: a LONG past 2^53; fl: a FLOAT; x: a DOUBLE with 0.0 and negative
# values; y: a DOUBLE with 0.0 (x / y meets 0 / 0 and x / 0); neg: negative; zero: 0.0; id / idr: unique (hash key space)
SCHEMA = [("g", "INT"), ("srt", "INT"), ("iv", "INT"), ("f", "INT"), ("a1", "INT"), ("a5", "INT"), ("a11", "INT"),
          ("vl", "LONG"), ("fl", "FLOAT"), ("x", "DOUBLE"), ("y", "DOUBLE"), ("neg", "DOUBLE"), ("zero", "DOUBLE"),
          ("id", "INT"), ("idr", "INT"), ("s", "STRING")]
DOCS = (70, 25003)
TOTAL = sum(DOCS)


def _columns(rng, n, id0):
    return {"g": rng.integers(0, 7, n), "srt": np.sort(rng.integers(0, 12, n)), "iv": rng.integers(0, 30, n),
            "f": rng.integers(0, 1000, n), "a1": rng.integers(0, 2, n) * 3, "a5": rng.integers(0, 20, n),
            "a11": rng.integers(0, 2000, n) - 1000, "vl": (1 << 60) + rng.integers(0, 4000, n).astype(np.int64) * 3 + 1,
            "fl": rng.uniform(-8, 8, n).astype(np.float32),
            "x": rng.integers(-4, 5, n).astype(np.float64) * 0.75, "y": rng.integers(-2, 3, n).astype(np.float64) * 0.5,
            "neg": -rng.uniform(1.0, 100.0, n), "zero": np.zeros(n), "id": np.arange(id0, id0 + n),
            "idr": np.arange(id0, id0 + n)[::-1].copy(), "s": ["s%02d" % v for v in rng.integers(0, 20, n)]}


def _dict_ids(values):
    return np.unique(np.asarray(values), return_inverse=True)[1]


def _pinned_form(oracle, cols):
    seg = oracle.make_segment(SCHEMA, cols)
    c = dict(seg.columns)
    c["iv"] = replace(c["iv"], inv_bytes=build_inverted_index(_dict_ids(cols["iv"]), c["iv"].cardinality))
    ids = _dict_ids(cols["srt"])
    c["srt"] = replace(c["srt"], fwd_bytes=_sorted_pairs(ids, c["srt"].cardinality), fwd_format=L.FWD_SORTED_PAIRS,
                       is_sorted=True)
    return SegmentBuffers(seg.num_docs, c)


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(29)
    cols = [_columns(rng, DOCS[0], 0), _columns(rng, DOCS[1], DOCS[0])]
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(_pinned_form(oracle, c)) for c in cols]
    allc = {name: (np.concatenate([c[name] for c in cols]) if typ != "STRING" else sum([c[name] for c in cols], []))
            for name, typ in SCHEMA}
    yield t, hs, cols, allc
    t.close()


# ------------------------------------------------------------------------------------------------ the numpy yardstick
def eval_np(tree, cols):
    """A tree's per-doc doubles, one numpy float64 operation per node in the reference's order (ADD / MULT: the folded
    literals first, then the other arguments in order)."""
    if tree[0] == "col":
        return np.asarray(cols[tree[1]]).astype(np.float64)
    if tree[0] == "lit":
        return np.float64(tree[1])
    fn, args = tree
    with np.errstate(all="ignore"):
        if fn == "sub":
            return eval_np(args[0], cols) - eval_np(args[1], cols)
        if fn == "div":
            return eval_np(args[0], cols) / eval_np(args[1], cols)
        acc = np.float64(0.0 if fn == "add" else 1.0)
        for a in args:
            if a[0] == "lit":
                acc = acc + np.float64(a[1]) if fn == "add" else acc * np.float64(a[1])
        for a in args:
            if a[0] != "lit":
                acc = acc + eval_np(a, cols) if fn == "add" else acc * eval_np(a, cols)
        return acc


def _bits(v):
    b = np.asarray(v, dtype=np.float64).view(np.uint64).copy()
    b[np.isnan(v)] = E.NAN_KEY  # Double.doubleToLongBits
    return b


def pred_mask(q, p, cols):
    """Java's raw DOUBLE evaluators over an expression's values (RANGE / EQ compare doubles: 0.0 == -0.0, a NaN matches
    neither; IN compares Double.doubleToLongBits); plain numeric comparison for a column."""
    expr = p.column in q.expressions
    v = eval_np(q.expressions[p.column], cols) if expr else np.asarray(cols[p.column]).astype(np.float64)
    lit = [None if s == "*" else float(s) for s in p.values]
    with np.errstate(invalid="ignore"):
        if p.type == "RANGE":
            m = np.ones(len(v), dtype=bool)
            if lit[0] is not None:
                m &= (v >= lit[0]) if p.lower_inclusive else (v > lit[0])
            if lit[1] is not None:
                m &= (v <= lit[1]) if p.upper_inclusive else (v < lit[1])
            return m
        if p.type in ("EQ", "NOT_EQ"):
            m = v == lit[0]
            return m if p.type == "EQ" else ~m
        m = np.isin(_bits(v), _bits(np.array(lit))) if expr else np.isin(v, lit)
        return m if p.type == "IN" else ~m


def filter_mask(q, f, cols):
    if f.type == "PREDICATE":
        return pred_mask(q, f.predicate, cols)
    kids = [filter_mask(q, k, cols) for k in f.children]
    if f.type == "NOT":
        return ~kids[0]
    return np.logical_and.reduce(kids) if f.type == "AND" else np.logical_or.reduce(kids)


def leaf_kind(q, p):
    if p.column in q.expressions:
        return "expr"
    if p.column == "srt":
        return "sorted"
    return "bitmap" if p.column == "iv" and p.type != "RANGE" else "scan"


def model_tree(q, f, cols, masks):
    """The reference's operator tree of filter f over one segment, folded as FilterPlanNode and FilterOperatorUtils fold
    it, for test_expr_filter_cpu's model.  A plain leaf that matches no doc is an EmptyFilterOperator and one that
    matches every doc a MatchAllFilterOperator (every dictionary value occurs in its segment, so the doc set tells);
    an expression leaf is never folded.  A NOT is a scan over what its operand does not match (the project's model)."""
    if f.type == "PREDICATE" or f.type == "NOT":
        m = filter_mask(q, f, cols)
        kind = leaf_kind(q, f.predicate) if f.type == "PREDICATE" else "scan"
        if f.type == "NOT":
            inner = model_tree(q, f.children[0], cols, [])
            if inner[0] in ("empty", "all"):
                return ("all",) if inner[0] == "empty" else ("empty",)
        elif kind != "expr" and (not m.any() or m.all()):
            return ("all",) if m.all() else ("empty",)
        masks.append(m)
        return (kind, len(masks) - 1)
    kids = [model_tree(q, k, cols, masks) for k in f.children]
    stop, skip = ("empty", "all") if f.type == "AND" else ("all", "empty")
    if any(k[0] == stop for k in kids):
        return (stop,)
    kids = [k for k in kids if k[0] != skip]
    if not kids:
        return (skip,)
    return kids[0] if len(kids) == 1 else ("and" if f.type == "AND" else "or", kids)


def model_stats(q, seg_cols):
    docs = entries = 0
    for cols in seg_cols:
        masks = []
        tree = model_tree(q, q.filter, cols, masks)
        docs += int(filter_mask(q, q.filter, cols).sum())
        if tree[0] not in ("empty", "all"):
            used = sorted({l[1] for l in M.leaves_of(tree)})  # (the leaves of folded branches are gone)
            renum = {old: new for new, old in enumerate(used)}
            entries += M.model_entries(_renumber(tree, renum), [masks[i] for i in used])
    return docs, entries


def _renumber(tree, renum):
    if tree[0] in ("and", "or"):
        return (tree[0], [_renumber(k, renum) for k in tree[1]])
    return (tree[0], renum[tree[1]])


def _q(where, select="COUNT(*), SUM(a5)", group_by="g", **kw):
    return parse_query("SELECT %s FROM t WHERE %s%s" % (select, where, " GROUP BY " + group_by if group_by else ""),
                       filter_expressions=True, **kw)


def check(t, hs, seg_cols, allc, q, path=None):
    """Rows (COUNT and the integer SUM(a5) per group), numDocsScanned and numEntriesScannedInFilter of q."""
    mask = filter_mask(q, q.filter, allc)
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        if path:
            assert p.group_path() == path
    keys = [np.asarray(allc[c])[mask].tolist() for c in q.group_by]
    a5 = np.asarray(allc["a5"])[mask].tolist()
    a11 = np.asarray(allc["a11"])[mask].tolist()
    want = {}
    for i in range(len(a5)):
        w = want.setdefault(tuple(k[i] for k in keys), [0, 0, -float("inf")])
        w[0] += 1
        w[1] += a5[i]
        w[2] = max(w[2], float(a11[i]))
    nagg = len(q.aggregations)  # COUNT(*), SUM(a5) and, where the query asks for it, MAX(a11)
    assert r.as_dict() == {k: w[:nagg] for k, w in want.items()}
    docs, entries = model_stats(q, seg_cols)
    assert docs == int(mask.sum())
    assert (r.stats.num_docs_scanned, r.stats.num_entries_scanned_in_filter) == (docs, entries)
    return r


# ------------------------------------------------------------------------------------------------ 1. every operator, alone
ALONE = ["a5 * a11 > 1000", "a5 * a11 >= 1000", "a5 * a11 < -3000", "a5 * a11 <= -3000", "a5 * a11 = 0",
         "a5 * a11 != 0", "a5 * a11 BETWEEN -500 AND 500.5", "a5 * a11 IN (0, 19, -19000, 7.5)",
         "a5 * a11 NOT IN (0, 38)", "a1 + a5 > 10", "(a1 - a11) / 4 <= 2.25", "vl - a11 > 1152921504606852000",
         "fl * 3 < -1.5", "ADD(x, y, 0.25) = 0.25", "x * neg - a5 / 7 > 3", "a11 / a5 > 100"]


@pytest.mark.parametrize("where", ALONE)
def test_alone(data, where):
    t, hs, seg_cols, allc = data
    q = _q(where)
    r = check(t, hs, seg_cols, allc, q, path="lds")
    assert r.stats.num_entries_scanned_in_filter == TOTAL  # a lone leaf evaluates every doc
    for h, cols in zip(hs, seg_cols):  # the doc set itself, through the standalone filter entry point
        got = np.unpackbits(t.filter_bitmap(h, q, len(cols["g"])).view(np.uint8), bitorder="little")[:len(cols["g"])]
        assert np.array_equal(got.astype(bool), filter_mask(q, q.filter, cols)), where


# ------------------------------------------------------------------------------------------------ 2. in company
COMPANY = [
    "f < 500 AND a5 * a11 > 1000",                       # AND with a scan: the leap-frog replay, blocks at targets
    "a5 * a11 > 1000 AND f < 20",                        # as written the other way round; few scan matches
    "srt BETWEEN 3 AND 7 AND a5 * a11 > 1000",           # a sorted leaf: applyAnd chain, counted in the kernel
    "iv IN (3, 4, 17) AND a5 * a11 <= 0",                # an inverted leaf
    "srt < 9 AND f >= 100 AND a5 * a11 != 0",            # sorted, scan, expression
    "iv = 5 AND srt > 2 AND a1 + a5 > 4 AND f < 900",    # the expression written before a scan: sorted after it
    "a5 * a11 > 15000 OR f < 30",                        # OR: every doc per scan-based child
    "a5 * a11 > 15000 OR iv = 7 OR srt = 11",
    "NOT a5 * a11 > 1000",
    "NOT (a5 * a11 > 1000 AND f < 500)",
    "a5 * a11 > 1000 AND a1 + a5 < 12",                  # two expression leaves
    "a5 * a11 > 1000 AND a5 * a11 < 9000 AND f < 700",
    "(f < 100 OR f > 900) AND a5 * a11 > 0",             # AND(OR(scan, scan), expr)
    "(f < 500 AND a5 * a11 > 1000) OR iv = 3",           # OR(AND(scan, expr), bitmap)
    "(a1 + a5) * 2 > 9 AND (g = 1 OR g = 2)",
]


@pytest.mark.parametrize("where", COMPANY)
def test_in_company(data, where):
    t, hs, seg_cols, allc = data
    check(t, hs, seg_cols, allc, _q(where), path="lds")


def test_beside_an_expression_aggregation(data):
    """SUM(a5 * a11) ... WHERE a5 * a11 > 10: one virtual column for both."""
    t, hs, seg_cols, allc = data
    q = parse_query("SELECT SUM(a5 * a11), MIN(x * neg), COUNT(*) FROM t WHERE a5 * a11 > 10 AND x * neg < 0 GROUP BY g",
                    filter_expressions=True)
    assert sorted(q.expressions) == ["mult(a5,a11)", "mult(x,neg)"]
    before = len(t.index)
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        assert p.scan_geometry()["variant"] in (12, 13)  # the scan's expression instances
    assert len(t.index) <= before + 2 and t.index["mult(a5,a11)"] >= len(SCHEMA)
    mask = filter_mask(q, q.filter, allc)
    s = E.group_stats([allc["g"]], eval_np(q.expressions["mult(a5,a11)"], allc), mask)
    m = E.group_stats([allc["g"]], eval_np(q.expressions["mult(x,neg)"], allc), mask)
    got = r.as_dict()
    assert set(got) == set(s)
    for k, (total, lo, cnt) in got.items():
        assert (total, E.bits(lo), cnt) == (s[k][0], E.bits(m[k][1]), s[k][3])  # integer products: an exact sum
    assert (r.stats.num_docs_scanned, r.stats.num_entries_scanned_in_filter) == model_stats(q, seg_cols)
    # the filter's operands are filter columns: g, a5, a11, x, neg are projected, each once
    assert r.stats.num_entries_scanned_post_filter == int(mask.sum()) * 5


# ------------------------------------------------------------------------------------------------ 3. Java's edge rules
def test_zeros_nans_and_infinities(data):
    t, hs, seg_cols, allc = data
    n_neg_zero = TOTAL  # neg * zero is -0.0 on every doc
    for where, want in [("neg * zero = 0", n_neg_zero), ("neg * zero >= 0", n_neg_zero), ("neg * zero < 0", 0),
                        ("neg * zero IN (0)", 0), ("neg * zero NOT IN (0)", n_neg_zero),
                        ("neg * zero IN (-0.0)", n_neg_zero), ("neg * zero BETWEEN -0.0 AND 0", n_neg_zero)]:
        q = _q(where, group_by=None)
        assert int(filter_mask(q, q.filter, allc).sum()) == want, where
        r = t.execute_aggregation(hs, q)
        assert r.values[0] == want and r.stats.num_docs_scanned == want, where
    x, y = allc["x"], allc["y"]
    nan, pinf, ninf = (x == 0) & (y == 0), (x > 0) & (y == 0), (x < 0) & (y == 0)
    assert nan.sum() > 100 and pinf.sum() > 100 and ninf.sum() > 100
    fin = y != 0
    with np.errstate(all="ignore"):
        quot = x / y
    for where, want in [("x / y >= -1e308", int((fin & (quot >= -1e308)).sum() + pinf.sum())),  # NaN matches no RANGE
                        ("x / y > -1e999", int(fin.sum() + pinf.sum())),     # the literal is -inf: exclusive of it
                        ("x / y >= -1e999", int(fin.sum() + pinf.sum() + ninf.sum())),
                        ("x / y < 1e999", int(fin.sum() + ninf.sum())),
                        ("x / y > 1e308", int(pinf.sum())), ("x / y < -1e308", int(ninf.sum())),
                        ("x / y = 0", int((fin & (x == 0)).sum())),
                        ("x / y != 0", int(TOTAL - (fin & (x == 0)).sum())),            # NaN matches every !=
                        ("x / y NOT IN (0, 1.5)", int(TOTAL - (fin & ((_bits(quot) == E.bits(0.0)) | (quot == 1.5))).sum())),
                        ("x / y IN (1.5, -1.5)", int((fin & (np.abs(quot) == 1.5)).sum()))]:
        q = _q(where, group_by=None)
        assert int(filter_mask(q, q.filter, allc).sum()) == want, where
        r = t.execute_aggregation(hs, q)
        assert r.values[0] == want and r.stats.num_entries_scanned_in_filter == TOTAL, where


# ------------------------------------------------------------------------------------------------ 4. post-filter entries
@pytest.mark.parametrize("expr, plain", [("a5 * 2 > 10", "a5 > 5"), ("f < 500 AND a5 + 0.5 <= 7.5", "f < 500 AND a5 <= 7"),
                                         ("srt < 9 AND a11 - a11 = 0", "srt < 9 AND g >= 0 AND a11 > -5000")])
def test_post_filter_entries_are_those_of_a_plain_predicate(data, expr, plain):
    t, hs, seg_cols, allc = data
    for select, group_by in (("COUNT(*), SUM(a5)", "g"), ("SUM(a11), MAX(x), MIN(vl)", "g, iv"), ("SUM(a11), COUNT(*)", None)):
        a = t.execute_groupby(hs, _q(expr, select, group_by))
        b = t.execute_groupby(hs, _q(plain, select, group_by))
        assert a.as_dict() == b.as_dict()
        assert a.stats.num_docs_scanned == b.stats.num_docs_scanned
        assert a.stats.num_entries_scanned_post_filter == b.stats.num_entries_scanned_post_filter


# ------------------------------------------------------------------------------------------------ 5. where it ran
def test_tables_and_pipelines(data):
    t, hs, seg_cols, allc = data
    where = "f < 600 AND a5 * a11 > -2000"
    check(t, hs, seg_cols, allc, _q(where), path="lds")
    t.set_config(lds_table_kb=1)
    try:
        check(t, hs, seg_cols, allc, _q(where, group_by="g, iv"), path="global")
    finally:
        t.reset_config()
    # 25073 x 25073 keys: the hash-partitioned pipeline, and with it switched off the scan's own hash table.  (Three
    # slots: the pipeline's one-word COUNT + SUM records give wrong rows on this table with or without an expression
    # leaf, with a plain predicate alone too -- a defect of that record form, older than this leaf and not its subject.)
    check(t, hs, seg_cols, allc, _q(where, select="COUNT(*), SUM(a5), MAX(a11)", group_by="id, idr",
                                    num_groups_limit=10 ** 9), path="hash_partitioned")
    t.set_config(hash_partitions=0)
    try:
        check(t, hs, seg_cols, allc, _q(where, group_by="id, idr", num_groups_limit=10 ** 9), path="hash")
    finally:
        t.reset_config()
    q = _q(where, select="COUNT(*), SUM(a5), MAX(vl)", group_by=None)  # aggregation-only
    r = t.execute_aggregation(hs, q)
    m = filter_mask(q, q.filter, allc)
    assert r.values == [int(m.sum()), float(allc["a5"][m].sum()), float(allc["vl"][m].max())]
    assert (r.stats.num_docs_scanned, r.stats.num_entries_scanned_in_filter) == model_stats(q, seg_cols)
    # the leaf beside DISTINCTCOUNT / PERCENTILE / exact_fp_sum plans
    q = _q(where, select="DISTINCTCOUNT(iv), PERCENTILE(a11, 50), COUNT(*)")
    plain = _q("f < 600 AND a11 > -5000", select="DISTINCTCOUNT(iv), PERCENTILE(a11, 50), COUNT(*)")
    got = t.execute_groupby(hs, q).as_dict()
    for k, (dc, pct, cnt) in got.items():
        sel = m & (allc["g"] == k[0])
        vals = np.sort(allc["a11"][sel])
        assert (dc, cnt) == (len(set(allc["iv"][sel].tolist())), int(sel.sum()))
        assert pct == float(vals[int(float(len(vals)) * 50.0 / 100.0)])
    assert set(got) == {(int(v),) for v in set(allc["g"][m].tolist())}
    assert plain.expressions == {}
    q = _q(where, select="SUM(x), COUNT(*)", exact_fp_sum=True)
    for k, (total, cnt) in t.execute_groupby(hs, q).as_dict().items():
        sel = m & (allc["g"] == k[0])
        assert (total, cnt) == (float(allc["x"][sel].sum()), int(sel.sum()))  # multiples of 0.75: exact in any order


def test_partitioned_pipeline(oracle, gpu_lib):
    """A dense key space that takes the radix-partitioned group-by, with an expression leaf in front of it."""
    schema = [("k1", "INT"), ("k2", "INT"), ("v", "INT"), ("w", "INT")]
    n = 20000
    rng = np.random.default_rng(9)
    cols = {"k1": rng.integers(0, 3000, n), "k2": rng.integers(0, 3000, n), "v": rng.integers(-9, 9, n),
            "w": rng.integers(1, 50, n)}
    cols["k1"][:3000] = np.arange(3000)
    cols["k2"][:3000] = np.arange(3000)
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        q = parse_query("SELECT SUM(v), COUNT(*) FROM t WHERE v * w > 20 GROUP BY k1, k2", num_groups_limit=10 ** 9,
                        filter_expressions=True)
        with t.plan([h], q) as p:
            assert p.group_path() == "partitioned"
            p.execute()
            r = p.finalize()
        m = cols["v"].astype(np.float64) * cols["w"].astype(np.float64) > 20
        want = {}
        for a, b, v in zip(cols["k1"][m].tolist(), cols["k2"][m].tolist(), cols["v"][m].tolist()):
            w = want.setdefault((a, b), [0, 0])
            w[0] += v
            w[1] += 1
        assert r.as_dict() == want
        assert (r.stats.num_docs_scanned, r.stats.num_entries_scanned_in_filter) == (int(m.sum()), n)


def test_segment_with_a_star_tree_is_scanned(oracle, gpu_lib):
    rng = np.random.default_rng(11)
    cols = SC.c4_columns(rng, 6000, cards=(12, 6, 5, 4))
    seg = oracle.make_segment(SC.C4_SCHEMA, cols)
    star = StarTree.build(SC.C4_SCHEMA, seg, SC.C4_SPLIT, SC.C4_PAIRS, max_leaf_records=100)
    with GpuTable(SC.C4_SCHEMA) as t:
        h = t.pin_segment(seg)
        t.attach_startree(h, star)
        with t.plan([h], parse_query("SELECT COUNT(*), SUM(m) FROM t WHERE d1 > 3 GROUP BY d4")) as p:
            p.execute()
            p.finalize()
            assert p.star_work()[0] == 1  # the control: a plain predicate on a dimension takes the star-tree
        q = parse_query("SELECT COUNT(*), SUM(m) FROM t WHERE d1 * 2 > 6 GROUP BY d4", filter_expressions=True)
        with t.plan([h], q) as p:
            p.execute()
            r = p.finalize()
            assert p.star_work()[0] == 0
        m = cols["d1"] > 3
        want = {(int(k),): [int((m & (cols["d4"] == k)).sum()), int(cols["m"][m & (cols["d4"] == k)].sum())]
                for k in set(cols["d4"][m].tolist())}
        assert r.as_dict() == want and r.stats.num_entries_scanned_in_filter == 6000


# ------------------------------------------------------------------------------------------------ 6. declined, errors
def test_declines_and_errors(data, oracle):
    t, hs, seg_cols, allc = data
    with pytest.raises(L.UnsupportedQueryError) as e:  # a STRING operand
        t.plan(hs, _q("a5 * s > 3"))
    assert "expression" in str(e.value) and "STRING" in str(e.value)
    mult = t.add_expression([(L.EXPR_COLUMN, t.index["a5"], 0.0), (L.EXPR_COLUMN, t.index["a11"], 0.0), (L.EXPR_MULT, 0, 0.0)])
    with pytest.raises(L.UnsupportedQueryError) as e:  # a virtual column nested as an operand
        t.add_expression([(L.EXPR_COLUMN, mult, 0.0), (L.EXPR_LITERAL, 0, 2.0), (L.EXPR_ADD, 0, 0.0)])
    assert "expression" in str(e.value) and "virtual" in str(e.value)
    # a virtual column in GROUP BY stays an invalid argument; so does a predicate column that names nothing
    q = parse_query("SELECT COUNT(*) FROM t WHERE a5 * a11 > 3 GROUP BY g", filter_expressions=True)
    to_c = q.to_c

    def group_by_virtual(index):
        c, keep = to_c(index)
        c.group_by[0] = mult
        return c, keep

    def predicate_nowhere(index):
        c, keep = to_c(index)
        c.predicates[0].column = len(SCHEMA) + 1000
        return c, keep

    for bad in (group_by_virtual, predicate_nowhere):
        q.to_c = bad
        with pytest.raises(L.PinotGpuError) as e:
            t.plan(hs, q)
        assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and "bad column" in str(e.value)
    # a literal that is no double
    with pytest.raises(L.PinotGpuError):
        t.plan(hs, QueryContext(["g"], [("COUNT", "*")], FilterContext.pred(Predicate.eq("a5 * a11", "abc"))))


def test_declined_raw_operand(oracle, gpu_lib):
    from pinot_amd.segment import build_raw_column
    schema = [("g", "INT"), ("v", "INT"), ("w", "LONG")]
    n = 64
    base = oracle.make_segment(schema[:2], {"g": np.arange(n) % 4, "v": np.arange(n)})
    cols = {**base.columns, "w": build_raw_column("LONG", (np.arange(n, dtype=np.int64) * 3).tolist(), 2)}
    with GpuTable(schema) as t:
        h = t.pin_segment(SegmentBuffers(n, cols))
        with pytest.raises(L.UnsupportedQueryError) as e:
            t.plan([h], parse_query("SELECT COUNT(*) FROM t WHERE v * w > 9 GROUP BY g", filter_expressions=True))
        assert "expression" in str(e.value) and "raw" in str(e.value)
        r = t.execute_groupby([h], parse_query("SELECT COUNT(*) FROM t WHERE v * 2 > 100 AND w > 30 GROUP BY g",
                                               filter_expressions=True))
        assert sum(v[0] for v in r.values) == int((np.arange(n) > 50).sum())  # beside a raw-value leaf it runs
