"""Arithmetic expressions inside aggregations on the GPU group-by path (SUM(price * qty)): the reference's recorded
answers (TransformQueriesTest.testTransformWithAvgInnerSegment, tests/golden/kat_transform_avg.json) and the
Python-float yardstick of expr_common.py -- the oracle has no transforms.  MIN, MAX and every per-doc value are compared
as bit patterns (a NaN as the canonical one); SUM and AVG sums exactly where the data makes them order-independent
(integer columns under + - *, every partial sum an integer below 2^53), else within the project's double-sum tolerance
of 1e-9, here relative to the sum of |terms|, so cancellation cannot hide an error.  Each test asserts through
Plan.group_path / Plan.scan_geometry()["variant"] (12 sparse, 13 dense: the expression instances of k_direct.hip) the
path it means to cover."""
import struct

import numpy as np
import pytest

import expr_common as E
import startree_common as SC
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import QueryContext, parse_query
from pinot_amd.startree import StarTree

pytestmark = pytest.mark.gpu
SPARSE, DENSE = 12, 13  # kScanExprSparse, kScanExprDense
TOL = 1e-9

# 8192 + 37 docs: one whole tile and a tail; 100 docs: a lane tail.  id is unique over both segments; f selects; a, b,
# c, d are integers (a and c negative in part); vl lies past 2^53, where (double)value rounds; fl is a FLOAT; x, y, z
# are full-mantissa doubles (a fused multiply-add rounds differently on most docs); n is negative, zero is 0.0.
SCHEMA = [("g1", "INT"), ("g2", "INT"), ("id", "INT"), ("f", "INT"), ("a", "INT"), ("b", "INT"), ("c", "INT"),
          ("d", "INT"), ("vl", "LONG"), ("fl", "FLOAT"), ("x", "DOUBLE"), ("y", "DOUBLE"), ("z", "DOUBLE"),
          ("n", "DOUBLE"), ("zero", "DOUBLE"), ("s", "STRING")]
DOCS = (8192 + 37, 100)


def _columns(rng, n, id0):
    return {"g1": rng.integers(0, 7, n), "g2": rng.integers(10, 15, n), "id": np.arange(id0, id0 + n),
            "f": rng.integers(0, 1000, n), "a": rng.integers(-500, 500, n), "b": rng.integers(1, 300, n),
            "c": rng.integers(-40, 40, n), "d": rng.integers(1, 9, n),
            "vl": (1 << 60) + rng.integers(0, 4000, n).astype(np.int64) * 3 + 1,
            "fl": rng.uniform(-8, 8, n).astype(np.float32), "x": rng.uniform(1.0, 2.0, n), "y": rng.uniform(-2.0, -1.0, n),
            "z": rng.uniform(-3.0, 3.0, n), "n": -rng.uniform(1.0, 100.0, n), "zero": np.zeros(n),
            "s": ["s%02d" % v for v in rng.integers(0, 20, n)]}


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(23)
    cols = [_columns(rng, DOCS[0], 0), _columns(rng, DOCS[1], DOCS[0])]
    segs = [oracle.make_segment(SCHEMA, c) for c in cols]
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(s) for s in segs]
    allc = {name: (np.concatenate([c[name] for c in cols]) if typ != "STRING" else sum([c[name] for c in cols], []))
            for name, typ in SCHEMA}
    yield t, hs, segs, allc
    t.close()


_DOC_CACHE = {}


def _docs(allc, expr):
    """The per-doc doubles of an expression over the whole table (computed once per expression)."""
    name = expr if isinstance(expr, str) else repr(expr)
    if name not in _DOC_CACHE:
        _DOC_CACHE[name] = E.eval_docs(expr, allc)
    return _DOC_CACHE[name]


def _run(t, hs, q):
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        return r, p.group_path(), p.scan_geometry()["variant"]


def _check_agg(fn, got, st, exact):
    """One aggregation's value against group statistics st = (sum, min, max, count, sum |terms|)."""
    s, lo, hi, cnt, mag = st
    if fn == "COUNT":
        assert got == cnt
    elif fn == "MIN":
        assert E.canon_bits(got) == E.canon_bits(lo)
    elif fn == "MAX":
        assert E.canon_bits(got) == E.canon_bits(hi)
    else:
        if fn == "AVG":
            assert got.count == cnt
            got = got.sum
        if exact or not np.isfinite(s):
            assert E.canon_bits(got) == E.canon_bits(s)
        else:
            assert abs(got - s) <= TOL * mag, (got, s, mag)


def _check_query(t, hs, allc, sql, mask, exact=False, path=None, variant=None):
    q = parse_query(sql) if isinstance(sql, str) else sql
    r, gpath, got_variant = _run(t, hs, q)
    assert got_variant == variant if variant is not None else got_variant in (SPARSE, DENSE)
    if path:
        assert gpath == path
    got = r.as_dict()
    stats = {}
    for fn, col in q.aggregations:
        if col not in stats:
            vals = np.zeros(len(mask)) if col == "*" else _docs(allc, q.expressions.get(col, col))
            stats[col] = E.group_stats([allc[c] for c in q.group_by], vals, mask)
    want = next(iter(stats.values()))
    assert set(got) == set(want)
    for k, row in got.items():
        for (fn, col), v in zip(q.aggregations, row):
            _check_agg(fn, v, stats[col][k], exact)
    assert r.stats.num_docs_scanned == int(np.asarray(mask).sum())
    return r


# ------------------------------------------------------------------------------------------------ 1. the reference's KAT
@pytest.fixture(scope="module")
def kat(oracle, gpu_lib):
    K = E.KAT_TRANSFORM
    schema = [tuple(x) for x in K["schema"]]
    cols = {name: ([K["row"][name]] * K["num_rows"] if typ == "STRING" else np.full(K["num_rows"], K["row"][name]))
            for name, typ in schema}
    t = GpuTable(schema)
    h = t.pin_segment(oracle.make_segment(schema, cols))
    yield t, h
    t.close()


@pytest.mark.parametrize("case", E.KAT_TRANSFORM["cases"], ids=lambda c: c["query"].split("FROM")[0][11:].strip())
def test_kat_transform_avg(kat, case):
    """TransformQueriesTest.java:148-168: (sum, count) per segment, and doubled over the segment taken twice."""
    t, h = kat
    q = parse_query(case["query"])
    for times in (1, 2):
        with t.plan([h] * times, q) as p:
            p.execute()
            res = p.finalize()
            assert p.scan_geometry()["variant"] == DENSE  # no filter
        (pair,), = res.values
        assert (pair.sum, pair.count) == (case["sum"] * times, case["count"] * times)
        assert res.stats.num_docs_scanned == 10 * times


@pytest.mark.parametrize("sql", E.KAT_TRANSFORM["failing"])
def test_kat_string_operand_is_declined(kat, sql):
    t, h = kat
    with pytest.raises(L.UnsupportedQueryError) as e:
        t.plan([h], parse_query(sql))
    assert "expression" in str(e.value) and "STRING" in str(e.value)


# ------------------------------------------------------------------------------------------------ 2. parity matrix
EXPRESSIONS = [("add", "a + b", True), ("sub", "SUB(a, c)", True), ("mult", "a * b", True), ("div", "a / d", False),
               ("nested", "ADD(DIV(a,b), DIV(c,d))", False), ("literals", "(2.5 - x) / 4 + 10 / (y - 0.5)", False),
               ("long_past_2p53", "vl - a", False), ("float", "fl * 3", False), ("double", "x * y + z", False),
               ("negative", "n * c - a", False)]


@pytest.mark.parametrize("group_by", [["g1"], ["g1", "g2"]], ids=["one_key", "two_keys"])
@pytest.mark.parametrize("f_below", [None, 60], ids=["all", "f6"])
@pytest.mark.parametrize("name, expr, exact", EXPRESSIONS, ids=[e[0] for e in EXPRESSIONS])
def test_parity(data, group_by, f_below, name, expr, exact):
    t, hs, segs, allc = data
    where = "" if f_below is None else " WHERE f < %d" % f_below
    mask = np.ones(len(allc["f"]), dtype=bool) if f_below is None else allc["f"] < f_below
    sql = "SELECT SUM(%s), MIN(%s), MAX(%s), AVG(%s), COUNT(%s) FROM t%s GROUP BY %s" % (
        (expr,) * 5 + (where, ", ".join(group_by)))
    r = _check_query(t, hs, allc, sql, mask, exact=exact, path="lds", variant=DENSE if f_below is None else SPARSE)
    if name == "long_past_2p53":  # the data does round: (double)value is not the value
        assert any(int(x) != v for x, v in zip(allc["vl"].astype(np.float64).tolist(), allc["vl"].tolist()))
    # numEntriesScannedPostFilter: docs x distinct group-by and expression columns
    ncols = len(set(group_by) | set(parse_query(sql).columns()) - {"f"})
    assert r.stats.as_tuple()[2] == int(mask.sum()) * ncols


# ------------------------------------------------------------------------------------------------ 3. per-doc exactness
def test_per_doc_values_are_exact(data):
    """GROUP BY the unique id: MIN = MAX = the doc's double and SUM = 0.0 + it, compared as bits."""
    t, hs, segs, allc = data
    fused = sum(E.fused_differs(x, y, z) for x, y, z in zip(allc["x"].tolist(), allc["y"].tolist(), allc["z"].tolist()))
    assert fused >= 1  # a contracted x * y + z would change bits on this data (on most docs, in fact)
    cases = [("x * y + z", None), ("ADD(MULT(n, zero), MULT(n, zero))", E.bits(0.0)),
             ("SUB(MULT(n, zero), zero)", E.bits(-0.0)), ("x / zero", E.bits(float("inf"))),
             ("n / zero", E.bits(float("-inf"))), ("zero / zero", E.NAN_KEY), ("z / x - y * y", None)]
    mask = np.ones(len(allc["id"]), dtype=bool)
    for expr, every in cases:
        q = parse_query("SELECT SUM(%s), MIN(%s), MAX(%s) FROM t GROUP BY id" % (expr, expr, expr))
        r, path, variant = _run(t, hs, q)
        assert variant == DENSE and path == "global"
        vals = _docs(allc, expr).tolist()
        got = r.as_dict()
        assert len(got) == len(vals)
        for i, v in enumerate(vals):
            s, lo, hi = got[(i,)]
            assert E.canon_bits(lo) == E.canon_bits(hi) == E.canon_bits(v)
            assert E.canon_bits(s) == E.canon_bits(0.0 + v)
            if every is not None:
                assert E.canon_bits(lo) == every
    # the two zeros are told apart by MIN / MAX across docs too: -0.0 sorts below +0.0
    q = parse_query("SELECT MIN(SUB(MULT(n, zero), zero)), MAX(ADD(MULT(n, zero), zero)), SUM(x / zero) FROM t")
    lo, hi, s = t.execute_aggregation(hs, q).values
    assert (E.bits(lo), E.bits(hi), s) == (E.bits(-0.0), E.bits(0.0), float("inf"))


# ------------------------------------------------------------------------------------------------ 4. where it ran
def test_instance_and_tables(data):
    t, hs, segs, allc = data
    allm = np.ones(len(allc["f"]), dtype=bool)
    sql = "SELECT SUM(a * b), MAX(x * y) FROM t%s GROUP BY g1"
    _check_query(t, hs, allc, sql % " WHERE f < 10", allc["f"] < 10, path="lds", variant=SPARSE)  # a selective filter
    _check_query(t, hs, allc, sql % "", allm, path="lds", variant=DENSE)                          # every doc
    _check_query(t, hs, allc, sql % " WHERE f < 150", allc["f"] < 150, path="lds", variant=SPARSE)
    t.set_config(dense_selectivity=0.1)
    try:  # the same query with dense_selectivity lowered (its lanes match ~5 of 32 docs), and a denser one
        _check_query(t, hs, allc, sql % " WHERE f < 150", allc["f"] < 150, path="lds", variant=DENSE)
        _check_query(t, hs, allc, sql % " WHERE f < 900", allc["f"] < 900, path="lds", variant=DENSE)
    finally:
        t.reset_config()
    t.set_config(lds_table_kb=1)  # the same query on the global table
    try:
        a = _check_query(t, hs, allc, "SELECT SUM(a * b), MIN(a * b), MAX(a * b) FROM t WHERE f < 500 GROUP BY g1, g2",
                         allc["f"] < 500, exact=True, path="global", variant=DENSE).as_dict()
        _check_query(t, hs, allc, "SELECT SUM(a * b), MIN(a * b), MAX(a * b) FROM t WHERE f < 50 GROUP BY g1, g2",
                     allc["f"] < 50, exact=True, path="global", variant=SPARSE)
    finally:
        t.reset_config()
    b = _check_query(t, hs, allc, "SELECT SUM(a * b), MIN(a * b), MAX(a * b) FROM t WHERE f < 500 GROUP BY g1, g2",
                     allc["f"] < 500, exact=True, path="lds", variant=DENSE).as_dict()
    assert a == b
    # a single-row (aggregation-only) table, filtered and not
    for where, m in ((" WHERE f < 300", allc["f"] < 300), ("", allm)):
        q = parse_query("SELECT SUM(a * b), MIN(x / y), MAX(vl - a), AVG(c - d), COUNT(*) FROM t" + where)
        _check_query(t, hs, allc, q, m)
        vals = t.execute_aggregation(hs, q).values
        st = E.group_stats([], _docs(allc, "a * b"), m)[()]
        assert vals[0] == st[0] and vals[4] == int(m.sum())
    none = t.execute_aggregation(hs, parse_query("SELECT SUM(a * b), MIN(a * b), MAX(a * b), AVG(a * b) FROM t WHERE f > 5000"))
    assert none.values[:3] == [0.0, float("inf"), float("-inf")] and none.values[3].count == 0


def test_hash_key_space(oracle, gpu_lib):
    """9000 x 9000 keys over 9000 docs: past every dense table, so the groups live in the hash table."""
    schema = [("h1", "INT"), ("h2", "INT"), ("v", "INT"), ("w", "DOUBLE")]
    n = 9000
    rng = np.random.default_rng(3)
    cols = {"h1": np.arange(n), "h2": np.arange(n)[::-1].copy(), "v": np.arange(n) % 50 - 20, "w": rng.uniform(1, 2, n)}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        q = parse_query("SELECT SUM(v * w), MIN(v * w), MAX(v - w), COUNT(*) FROM t GROUP BY h1, h2", num_groups_limit=10 ** 9)
        r, path, variant = _run(t, [h], q)
        assert path == "hash" and variant == SPARSE  # (dense key spaces only have the whole-group instance)
        got = r.as_dict()
        m1, m2 = E.eval_docs("v * w", cols).tolist(), E.eval_docs("v - w", cols).tolist()
        assert len(got) == n
        for i in range(n):
            s, lo, hi, c = got[(i, n - 1 - i)]
            assert (E.bits(s), E.bits(lo), E.bits(hi), c) == (E.bits(0.0 + m1[i]), E.bits(m1[i]), E.bits(m2[i]), 1)


# ------------------------------------------------------------------------------------------------ 5. lane and tile edges
@pytest.mark.parametrize("ids", [[0], [31], [32 * 255 + 31], [8191, 8192], [0, 31, 8191, 8192, 8228],
                                 [8229, 8229 + 99], [8229 + 64]],
                         ids=["first_lane", "first_lane_end", "last_lane", "tile_boundary", "both_tiles",
                              "small_segment_ends", "small_segment_only"])
def test_matched_docs_at_the_edges(data, ids):
    t, hs, segs, allc = data
    q = parse_query("SELECT SUM(x * y + z), MIN(a * b), MAX(a * b), COUNT(*) FROM t WHERE id IN (%s) GROUP BY g1"
                    % ", ".join(str(i) for i in ids))
    mask = np.isin(allc["id"], ids)
    assert int(mask.sum()) == len(ids)
    _check_query(t, hs, allc, q, mask)


# ------------------------------------------------------------------------------------------------ 6 / 7. company, entries
def test_shared_evaluation_and_company(data):
    t, hs, segs, allc = data
    sql = "SELECT SUM(a*b), COUNT(*), MAX(a*b), SUM(a), AVG(a*b), MIN(c-d) FROM t WHERE f < 200 GROUP BY g1, g2"
    r = _check_query(t, hs, allc, sql, allc["f"] < 200, exact=True, path="lds")
    with t.plan(hs, parse_query(sql)) as p:
        ns, nk, kinds = p.layout()
        # COUNT, the sum and the max of a * b (AVG shares the sum), SUM(a), MIN(c - d)
        assert kinds == [L.SLOT_COUNT, L.SLOT_SUM_F64, L.SLOT_MAX_KEY, L.SLOT_SUM_I64, L.SLOT_MIN_KEY]
    m = int((allc["f"] < 200).sum())
    assert r.stats.as_tuple()[2] == m * 6  # g1, g2, a, b, c, d


def test_entries_scanned_post_filter(data):
    t, hs, segs, allc = data
    for where, m in ((" WHERE f < 200", allc["f"] < 200), ("", np.ones(len(allc["f"]), dtype=bool))):
        r = _check_query(t, hs, allc, "SELECT SUM(a*b), SUM(a) FROM t%s GROUP BY g1" % where, m, exact=True)
        assert r.stats.as_tuple()[2] == int(m.sum()) * 3  # g1, a, b: each column once


# ------------------------------------------------------------------------------------------------ 8. registration
def test_registration(data):
    t, hs, segs, allc = data
    ncols = len(SCHEMA)
    ia, ib = t.index["a"], t.index["b"]
    prog = [(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_COLUMN, ib, 0.0), (L.EXPR_SUB, 0, 0.0), (L.EXPR_LITERAL, 0, 0.75),
            (L.EXPR_DIV, 0, 0.0)]
    c1 = t.add_expression(prog, "div(sub(a,b),0.75)")
    c2 = t.add_expression(prog, "another name")
    c3 = t.add_expression(prog[:3])
    assert c1 == c2 >= ncols and c3 >= ncols and c3 != c1
    assert t.expression(c1) == (prog, "div(sub(a,b),0.75)")
    assert t.expression(c3) == (prog[:3], "sub(a,b)")  # the name built from the program
    with pytest.raises(L.PinotGpuError):
        t.expression(ia)
    # the Python layer registers on first use, once per expression
    q = parse_query("SELECT SUM((a - b) / 0.75), MAX(DIV(MINUS(a, b), 0.75)) FROM t GROUP BY g1")
    with t.plan(hs, q):
        pass
    assert t.index["div(sub(a,b),0.75)"] == c1
    # COUNT of a column index that names nothing (the Python layer never sends one)
    q = parse_query("SELECT COUNT(*), SUM(a) FROM t GROUP BY g1")
    to_c = q.to_c

    def bad(index):
        c, keep = to_c(index)
        c.aggs[0].column = ncols + 1000
        return c, keep

    q.to_c = bad
    with pytest.raises(L.PinotGpuError) as e:
        t.plan(hs, q)
    assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and "bad column" in str(e.value)
    # the ABI's own checks
    bad = [([(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_ADD, 0, 0.0)], "underflow"),
           ([(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_COLUMN, ib, 0.0)], "one value"),
           ([(L.EXPR_COLUMN, ia, 0.0)] + [(L.EXPR_COLUMN, ib, 0.0), (L.EXPR_ADD, 0, 0.0)] * 8, "1 to 16"),
           ([(L.EXPR_COLUMN, ia, 0.0)] * 5 + [(L.EXPR_ADD, 0, 0.0)] * 4, "deeper"),
           (sum([[(L.EXPR_COLUMN, i, 0.0)] + ([(L.EXPR_ADD, 0, 0.0)] if i else []) for i in range(5)], []), "4 distinct"),
           ([(L.EXPR_LITERAL, 0, 1.0), (L.EXPR_LITERAL, 0, 2.0), (L.EXPR_ADD, 0, 0.0)], "no column"),
           ([(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_COLUMN, 9999, 0.0), (L.EXPR_ADD, 0, 0.0)], "bad column"),
           ([(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_COLUMN, ib, 0.0), (77, 0, 0.0)], "unknown op")]
    for ops, word in bad:
        with pytest.raises(L.PinotGpuError) as e:
            t.add_expression(ops)
        assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and word in str(e.value), str(e.value)
    for ops, word in (([(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_COLUMN, c1, 0.0), (L.EXPR_ADD, 0, 0.0)], "virtual"),
                      ([(L.EXPR_COLUMN, ia, 0.0), (L.EXPR_COLUMN, t.index["s"], 0.0), (L.EXPR_ADD, 0, 0.0)], "STRING")):
        with pytest.raises(L.UnsupportedQueryError) as e:
            t.add_expression(ops)
        assert "expression" in str(e.value) and word in str(e.value)


# ------------------------------------------------------------------------------------------------ 9 / 10. hygiene
def test_reexecution_and_plan_cache(data):
    t, hs, segs, allc = data
    sql = "SELECT SUM(a * b), MIN(x * y), COUNT(*) FROM t WHERE f %s 400 GROUP BY g1"
    q, q2 = parse_query(sql % "<"), parse_query(sql % ">=")
    with t.plan(hs, q) as p:
        p.execute()
        p.execute()  # the table starts over with every execution: no doubled sums
        twice = p.finalize().as_dict()
    a = _check_query(t, hs, allc, q, allc["f"] < 400, exact=True).as_dict()
    b = _check_query(t, hs, allc, q2, allc["f"] >= 400, exact=True).as_dict()
    c = t.execute_groupby(hs, parse_query(sql % "<")).as_dict()  # a plan-cache hit
    assert twice == a == c and a != b


def test_two_plans_in_flight_on_two_streams(data):
    import torch
    t, hs, segs, allc = data
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    q1 = parse_query("SELECT SUM(a * b), MAX(a - c) FROM t WHERE f < 150 GROUP BY g1, g2")
    q2 = parse_query("SELECT SUM(a * b), MAX(a - c) FROM t WHERE f >= 150 GROUP BY g1, g2")
    p1 = t.plan_execute(hs, q1, stream=s1.cuda_stream)
    p2 = t.plan_execute(hs, q2, stream=s2.cuda_stream)
    try:
        r2 = p2.finalize(s2.cuda_stream).as_dict()
        r1 = p1.finalize(s1.cuda_stream).as_dict()
    finally:
        p1.close()
        p2.close()
    for got, m in ((r1, allc["f"] < 150), (r2, allc["f"] >= 150)):
        s = E.group_stats([allc["g1"], allc["g2"]], _docs(allc, "a * b"), m)
        x = E.group_stats([allc["g1"], allc["g2"]], _docs(allc, "a - c"), m)
        assert got == {k: [s[k][0], x[k][2]] for k in s}
    assert r1 != r2


# ------------------------------------------------------------------------------------------------ 11. star-tree
def test_segment_with_a_star_tree_is_scanned(oracle, gpu_lib):
    rng = np.random.default_rng(11)
    cols = SC.c4_columns(rng, 6000, cards=(12, 6, 5, 4))
    seg = oracle.make_segment(SC.C4_SCHEMA, cols)
    star = StarTree.build(SC.C4_SCHEMA, seg, SC.C4_SPLIT, SC.C4_PAIRS, max_leaf_records=100)
    with GpuTable(SC.C4_SCHEMA) as t:
        h = t.pin_segment(seg)
        t.attach_startree(h, star)
        with t.plan([h], parse_query("SELECT COUNT(*), SUM(m) FROM t GROUP BY d4")) as p:
            p.execute()
            p.finalize()
            assert p.star_work()[0] == 1  # the control: the same shape without an expression takes the star-tree
        with t.plan([h], parse_query("SELECT COUNT(*), SUM(m * 2), MAX(m - md) FROM t GROUP BY d4")) as p:
            p.execute()
            r = p.finalize()
            assert p.star_work()[0] == 0 and p.scan_geometry()["variant"] == DENSE
        allm = np.ones(6000, dtype=bool)
        s = E.group_stats([cols["d4"]], E.eval_docs("m * 2", cols), allm)
        x = E.group_stats([cols["d4"]], E.eval_docs("m - md", cols), allm)
        assert r.as_dict() == {k: [s[k][3], s[k][0], x[k][2]] for k in s}
        assert r.stats.num_docs_scanned == 6000


# ------------------------------------------------------------------------------------------------ 12. ORDER BY
def test_order_by_expression_desc_limit(data):
    t, hs, segs, allc = data
    q = parse_query("SELECT g1, g2, SUM(a*b) FROM t WHERE f < 300 GROUP BY g1, g2 ORDER BY SUM(a*b) DESC LIMIT 3")
    q.min_server_group_trim_size = 1  # the server keeps max(limit * 5, 1) = 15 groups
    top = t.execute_groupby(hs, q).trim_sql()
    st = E.group_stats([allc["g1"], allc["g2"]], _docs(allc, "a * b"), allc["f"] < 300)
    order = sorted(st.items(), key=lambda kv: (-kv[1][0], kv[0][1], kv[0][0]))
    assert len(top) == 15
    assert top.keys[:3] == [k for k, _ in order[:3]]
    assert [v[0] for v in top.values[:3]] == [v[0] for _, v in order[:3]]


# ------------------------------------------------------------------------------------------------ 13. the limits
def test_program_at_the_limits(data):
    """15 ops -- the longest well-formed program within 16 (k operands take k - 1 binary ops) -- at depth 4 over 4
    columns; then a 13-op program of the Python layer (its n-ary forms spend an op on the folded literal)."""
    t, hs, segs, allc = data
    ix = [t.index[c] for c in ("x", "y", "z", "n")]
    C, A, S, M, D = L.EXPR_COLUMN, L.EXPR_ADD, L.EXPR_SUB, L.EXPR_MULT, L.EXPR_DIV
    prog = [(C, ix[0], 0.0), (C, ix[1], 0.0), (C, ix[2], 0.0), (C, ix[3], 0.0), (A, 0, 0.0), (A, 0, 0.0), (A, 0, 0.0),
            (C, ix[0], 0.0), (M, 0, 0.0), (C, ix[1], 0.0), (S, 0, 0.0), (C, ix[2], 0.0), (D, 0, 0.0),
            (L.EXPR_LITERAL, 0, 2.0), (M, 0, 0.0)]
    col = t.add_expression(prog, "limits")
    t.index["limits"] = col
    x, y, z, n = (allc[c].tolist() for c in ("x", "y", "z", "n"))
    vals = np.array([((((a + (b + (c + d))) * a) - b) / c) * 2.0 for a, b, c, d in zip(x, y, z, n)])
    q = QueryContext(["id"], [("MIN", "limits"), ("MAX", "limits")])
    got = _run(t, hs, q)[0].as_dict()
    for i, v in enumerate(vals.tolist()):
        assert [E.bits(g) for g in got[(i,)]] == [E.bits(v)] * 2
    mask = allc["f"] < 500
    _check_query(t, hs, allc, "SELECT SUM(x + y * z - n / x), MIN(ADD(x, y, z, n, 1, 2)) FROM t WHERE f < 500 "
                 "GROUP BY g1", mask)


# ------------------------------------------------------------------------------------------------ 14. declined shapes
def _declined(fn):
    with pytest.raises(L.UnsupportedQueryError) as e:
        fn()
    assert "expression" in str(e.value), str(e.value)


def test_declined_shapes(data):
    import torch
    t, hs, segs, allc = data
    _declined(lambda: t.plan(hs, parse_query("SELECT DISTINCTCOUNT(a * b) FROM t GROUP BY g1")))
    _declined(lambda: t.plan(hs, parse_query("SELECT PERCENTILE(a * b, 50) FROM t GROUP BY g1")))
    _declined(lambda: t.plan(hs, parse_query("SELECT SUM(a * b), DISTINCTCOUNT(c) FROM t GROUP BY g1")))
    _declined(lambda: t.plan(hs, parse_query("SELECT SUM(a * b), PERCENTILE50(c) FROM t GROUP BY g1")))
    _declined(lambda: t.plan(hs, parse_query("SELECT SUM(x * y) FROM t GROUP BY g1", exact_fp_sum=True)))
    _declined(lambda: t.fp_sum_ranges(hs, parse_query("SELECT SUM(x * y) FROM t GROUP BY g1", exact_fp_sum=True)))
    _declined(lambda: t.plan(hs, parse_query("SELECT SUM(a * s) FROM t GROUP BY g1")))
    # numGroupsLimit plans that split per segment
    q = QueryContext(["id"], [("COUNT", "*"), ("SUM", "a * b")], None, num_groups_limit=1000)
    _declined(lambda: t.plan(hs, q))
    _declined(lambda: t.execute_groupby(hs, q))
    # an external table: create_execute, execute, finalize, combine
    d = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    q = parse_query("SELECT COUNT(*), SUM(a * b) FROM t GROUP BY g1, g2")
    _declined(lambda: t.plan_execute(hs, q, d_table=d.data_ptr()))
    with t.plan(hs, q) as p:
        _declined(lambda: p.execute(None, d.data_ptr()))
        p.execute()
        _declined(lambda: p.finalize(None, d.data_ptr()))
    # more distinct expressions than one plan holds
    many = ", ".join("SUM(a * %d.5)" % i for i in range(9))
    _declined(lambda: t.plan(hs, parse_query("SELECT %s FROM t GROUP BY g1" % many)))


def test_declined_raw_operand(oracle, gpu_lib):
    from pinot_amd.segment import SegmentBuffers, build_raw_column
    schema = [("g", "INT"), ("v", "INT"), ("w", "LONG")]
    n = 64
    base = oracle.make_segment(schema[:2], {"g": np.arange(n) % 4, "v": np.arange(n)})
    cols = {**base.columns, "w": build_raw_column("LONG", (np.arange(n, dtype=np.int64) * 3).tolist(), 2)}
    with GpuTable(schema) as t:
        h = t.pin_segment(SegmentBuffers(n, cols))
        _declined(lambda: t.plan([h], parse_query("SELECT SUM(v * w) FROM t GROUP BY g")))
        with t.plan([h], parse_query("SELECT SUM(v * 2) FROM t GROUP BY g")) as p:
            assert p.scan_geometry()["variant"] == DENSE


def test_partitioned_pipelines_are_not_taken(oracle, gpu_lib):
    """A dense key space large enough for the radix-partitioned group-by: an expression plan keeps the scan's own
    global table (planned as with partitioned_group_by = 0)."""
    schema = [("k1", "INT"), ("k2", "INT"), ("v", "INT")]
    n = 20000
    rng = np.random.default_rng(9)
    cols = {"k1": rng.integers(0, 3000, n), "k2": rng.integers(0, 3000, n), "v": rng.integers(-9, 9, n)}
    cols["k1"][:3000] = np.arange(3000)
    cols["k2"][:3000] = np.arange(3000)
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        with t.plan([h], parse_query("SELECT SUM(v) FROM t GROUP BY k1, k2", num_groups_limit=10 ** 9)) as p:
            control = p.group_path()
        q = parse_query("SELECT SUM(v * 3), COUNT(*) FROM t GROUP BY k1, k2", num_groups_limit=10 ** 9)
        r, path, variant = _run(t, [h], q)
        assert control == "partitioned" and path == "global" and variant == DENSE
        st = E.group_stats([cols["k1"], cols["k2"]], E.eval_docs("v * 3", cols), np.ones(n, dtype=bool))
        assert r.as_dict() == {k: [s[0], s[3]] for k, s in st.items()}


def test_hash_partitioned_pipeline_is_not_taken(oracle, gpu_lib):
    """A sparse key space below 2^31 (3000 x 3000 x 30), which a plain query aggregates per hash partition: an expression
    plan keeps the scan's own hash table (planned as with hash_partitions = 0)."""
    schema = [("a", "INT"), ("b", "INT"), ("c", "INT"), ("m", "INT")]
    n = 30000
    rng = np.random.default_rng(41)
    cols = {"a": rng.integers(0, 3000, n), "b": rng.integers(0, 3000, n), "c": rng.integers(0, 30, n),
            "m": rng.integers(-400, 900, n)}
    for name, card in (("a", 3000), ("b", 3000), ("c", 30)):
        cols[name][:card] = np.arange(card)
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        with t.plan([h], parse_query("SELECT SUM(m), COUNT(*) FROM t GROUP BY a, b, c", num_groups_limit=10 ** 9)) as p:
            control = p.group_path()
        q = parse_query("SELECT SUM(m * 3), MAX(m - c), COUNT(*) FROM t GROUP BY a, b, c", num_groups_limit=10 ** 9)
        r, path, variant = _run(t, [h], q)
        assert control == "hash_partitioned" and path == "hash" and variant == SPARSE
        allm = np.ones(n, dtype=bool)
        keys = [cols["a"], cols["b"], cols["c"]]
        s = E.group_stats(keys, E.eval_docs("m * 3", cols), allm)
        x = E.group_stats(keys, E.eval_docs("m - c", cols), allm)
        assert r.as_dict() == {k: [s[k][0], x[k][2], s[k][3]] for k in s}


def test_streamed_launches_are_not_taken(oracle, gpu_lib):
    """stream_chunks = 4 over 8 segments: a plain plan created and executed in one call runs as several launches (its
    last launch covers a part of the tiles), an expression plan as one (planned as with stream_chunks = 1)."""
    schema = [("g", "INT"), ("v", "INT"), ("w", "INT")]
    rng = np.random.default_rng(5)
    cols = [{"g": rng.integers(0, 9, 700), "v": rng.integers(-50, 50, 700), "w": rng.integers(1, 20, 700)} for _ in range(8)]
    allc = {k: np.concatenate([c[k] for c in cols]) for k in ("g", "v", "w")}
    with GpuTable(schema, config={"stream_chunks": 4, "plan_cache": 0}) as t:
        hs = [t.pin_segment(oracle.make_segment(schema, c)) for c in cols]
        with t.plan_execute(hs, parse_query("SELECT SUM(v), COUNT(*) FROM t GROUP BY g")) as p:
            p.finalize()
            geo = p.scan_geometry()
            assert geo["launch_tiles"] < geo["tiles"]  # the control: streamed
        with t.plan_execute(hs, parse_query("SELECT SUM(v * w), MIN(v - w), COUNT(*) FROM t GROUP BY g")) as p:
            r = p.finalize()
            geo = p.scan_geometry()
            assert geo["launch_tiles"] == geo["tiles"] and geo["variant"] == DENSE
        allm = np.ones(len(allc["g"]), dtype=bool)
        s = E.group_stats([allc["g"]], E.eval_docs("v * w", allc), allm)
        x = E.group_stats([allc["g"]], E.eval_docs("v - w", allc), allm)
        assert r.as_dict() == {k: [s[k][0], x[k][1], s[k][3]] for k in s}


# ------------------------------------------------------------------------------------------------ 15. DataTable
def test_datatable_names_the_expression(data):
    t, hs, segs, allc = data
    q = parse_query("SELECT SUM(a * b), MAX(ADD(DIV(a, b), 2.5)), COUNT(*) FROM t WHERE f < 100 GROUP BY g1")
    res = t.execute_groupby(hs, q)
    raw = res.datatable()
    assert b"sum(mult(a,b))" in raw and b"max(add(div(a,b),2.5))" in raw and b"count(*)" in raw
    for row in res.values:
        assert struct.pack(">d", row[0]) in raw and struct.pack(">d", row[1]) in raw
    st = E.group_stats([allc["g1"]], _docs(allc, "a * b"), allc["f"] < 100)
    assert {k: v[0] for k, v in res.as_dict().items()} == {k: s[0] for k, s in st.items()}


# ------------------------------------------------------------------------------------------------ 16. one-rank combine
def test_one_rank_host_communicator(data):
    from pinot_amd.combine import Communicator, combine_mode, combine_plan
    t, hs, segs, allc = data
    q = parse_query("SELECT COUNT(*), SUM(a * b), MIN(x * y), MAX(x * y) FROM t WHERE f < 500 GROUP BY g1, g2")
    want = _check_query(t, hs, allc, q, allc["f"] < 500, exact=False).as_dict()
    comm = Communicator(L.COMM_HOST, Communicator.unique_id(L.COMM_HOST), 1, 0, 0)
    try:
        with t.plan(hs, q) as p:
            p.execute()
            mode, kinds = combine_mode(p, comm, 1 << 62)
            assert mode == L.COMBINE_ALL_REDUCE
            assert kinds == [L.SLOT_COUNT, L.SLOT_SUM_F64, L.SLOT_MIN_KEY, L.SLOT_MAX_KEY]
            combine_plan(p, comm, None, mode, kinds)
            got = p.finalize().as_dict()
    finally:
        comm.close()
    assert set(got) == set(want)
    for k in want:
        assert got[k][0] == want[k][0] and [E.bits(v) for v in got[k][2:]] == [E.bits(v) for v in want[k][2:]]
        assert got[k][1] == want[k][1]  # integer products: the sum is order-independent
