"""Conditional aggregation on the GPU group-by path: CASE WHEN inside aggregations and on a predicate's left, against the
typed numpy yardstick of case_common.py (the reference's typing rules restated; it never calls the compiler under
test).  Per-doc values are read by grouping on the unique id, so MIN = MAX = the doc's value, and compared as bit
patterns (a NaN as the canonical one); sums are exact where they are integers below 2^53, else within the project's
1e-9 relative to the sum of |terms|.  Shapes as in test_expr_agg_gpu.py, for its reasons: segments of 8192 + 37 docs (a
whole tile and a tail) and 100 docs (a lane tail), and one segment of a single doc.  Each test asserts the path it means
to cover through Plan.group_path / Plan.scan_geometry()["variant"] (12 sparse, 13 dense: the expression instances)."""
import numpy as np
import pytest

import case_common as C
import expr_common as E
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import expr_columns, parse_query

pytestmark = pytest.mark.gpu
SPARSE, DENSE = 12, 13
TOL = 1e-9

# id is unique over the segments; f selects; i, j are small INTs; l is a LONG within +-2^53 (some values at 2^52), big a
# LONG past 2^53; fl a FLOAT holding (float)0.1 and its neighbour; d and e DOUBLEs holding -0.0, +0.0, NaN, +-inf and
# values that differ only below float precision (0.1, (double)(float)0.1, the double after 0.1); x a full-mantissa
# DOUBLE; q a positive INT.
SCHEMA = [("g1", "INT"), ("g2", "INT"), ("id", "INT"), ("f", "INT"), ("i", "INT"), ("j", "INT"), ("l", "LONG"),
          ("big", "LONG"), ("fl", "FLOAT"), ("d", "DOUBLE"), ("e", "DOUBLE"), ("x", "DOUBLE"), ("q", "INT")]
DOCS = (8192 + 37, 100, 1)
F01 = float(np.float32(0.1))  # 0.10000000149011612
SPECIAL = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.1, F01, 0.10000000000000002, 0.09999999999999999,
           1.0, -1.0, 2.5, 1e300, -1e-300]
FLOATS = [0.1, float(np.nextafter(np.float32(0.1), np.float32(1))), 0.3, -2.5, 0.0, 2.5]


def _columns(rng, n, id0):
    l = rng.integers(0, 300, n).astype(np.int64)
    l[rng.random(n) < 0.05] += 1 << 52
    return {"g1": rng.integers(0, 7, n), "g2": rng.integers(10, 15, n), "id": np.arange(id0, id0 + n),
            "f": rng.integers(0, 1000, n), "i": rng.integers(-3, 4, n), "j": rng.integers(-3, 4, n), "l": l,
            "big": (1 << 60) + rng.integers(0, 4000, n).astype(np.int64) * 3 + 1,
            "fl": rng.choice(FLOATS, n).astype(np.float32), "d": rng.choice(SPECIAL, n), "e": rng.choice(SPECIAL, n),
            "x": rng.uniform(1.0, 2.0, n), "q": rng.integers(1, 9, n)}


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(31)
    cols, id0 = [], 0
    for n in DOCS:
        cols.append(_columns(rng, n, id0))
        id0 += n
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(oracle.make_segment(SCHEMA, c)) for c in cols]
    allc = C.typed({name: np.concatenate([c[name] for c in cols]) for name, _ in SCHEMA}, SCHEMA)
    yield t, hs, allc
    t.close()


_DOC_CACHE = {}


def _tree(expr):
    return parse_query("SELECT SUM(%s) FROM t" % expr).expressions.popitem()[1]


def _docs(allc, tree):
    """The yardstick's per-doc doubles of a tree over the whole table (computed once per expression)."""
    name = repr(tree)
    if name not in _DOC_CACHE:
        _DOC_CACHE[name] = C.eval_docs(tree, allc)
    return _DOC_CACHE[name]


def _run(t, hs, q):
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        return r, p.group_path(), p.scan_geometry()["variant"]


def _check_agg(fn, got, st, exact):
    """One aggregation's value against group statistics st = (sum, min, max, count, sum |terms|); exact: every term is
    an integer (and the sum of their magnitudes below 2^53), so the sum does not depend on the order."""
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
        if not np.isfinite(s) or (exact and mag < 2.0 ** 53):
            assert E.canon_bits(got) == E.canon_bits(s)
        else:
            assert abs(got - s) <= TOL * mag, (got, s, mag)


def _check_query(t, hs, allc, sql, mask, path=None, variant=None):
    q = parse_query(sql, filter_expressions=True) if isinstance(sql, str) else sql
    r, gpath, got_variant = _run(t, hs, q)
    if variant is not None:
        assert got_variant == variant
    if path:
        assert gpath == path
    got = r.as_dict()
    stats = {}
    for fn, col in q.aggregations:
        if col not in stats:
            vals = np.zeros(len(mask)) if col == "*" else \
                _docs(allc, q.expressions[col]) if col in q.expressions else allc[col].astype(np.float64)
            with np.errstate(invalid="ignore"):
                whole = bool(np.all(vals[np.asarray(mask)] == np.floor(vals[np.asarray(mask)])))
            stats[col] = (E.group_stats([allc[c] for c in q.group_by], vals, mask), whole)
    want = next(iter(stats.values()))[0]
    assert set(got) == set(want)
    for k, row in got.items():
        for (fn, col), v in zip(q.aggregations, row):
            _check_agg(fn, v, stats[col][0][k], stats[col][1])
    assert r.stats.num_docs_scanned == int(np.asarray(mask).sum())
    return r


# name -> expression: one and three WHENs, AND / OR conditions, arithmetic in THEN and in a condition, a CASE inside
# arithmetic, R = FLOAT with literals, the total order's special values
CASES = {
    "one_when": "CASE WHEN i = 3 THEN x ELSE 0 END",
    "three_whens": "CASE WHEN l > 100 THEN 1 WHEN l > 10 THEN 0.5 ELSE 0 END",
    "and": "CASE WHEN i > 0 AND j < 2 THEN x ELSE e END",
    "or": "CASE WHEN i > 2 OR fl <= 0.1 THEN x ELSE 0.1 END",
    "and_or": "CASE WHEN i > 1 AND (j < 0 OR q > 6) THEN 1 ELSE 0 END",
    "arith_then_and_cond": "CASE WHEN i * j > 2 THEN x / q ELSE 0 END",
    "div_by_zero_unselected": "CASE WHEN e > 0 THEN x / e ELSE 0 END",
    "case_times": "CASE WHEN i > 0 THEN x ELSE 0.5 END * q",
    "case_minus": "CASE WHEN d > 0.1 THEN fl ELSE 0.1 END - j",
    "float_result": "CASE WHEN d > 0.1 THEN 0.1 ELSE 0.0 END",
    "double_literal": "CASE WHEN d > 0.10000000075 THEN 0.5 ELSE e END",
    "zero_signs_and_nans": "CASE WHEN d = e THEN 1 ELSE 0 END",
    "total_order": "CASE WHEN d > e THEN 1 WHEN d < e THEN -1 ELSE 0 END",
    "positive_zero_literal": "CASE WHEN d = 0.0 THEN 1 WHEN d <= -0.0 THEN 2 ELSE 3 END",
    "long_result": "CASE WHEN d >= 1 THEN i WHEN l >= 4503599627370496 THEN l ELSE 7 END",
    "int_columns": "CASE WHEN i >= j THEN i ELSE j END",
    "nested_else": "CASE WHEN i > 1 THEN 3 ELSE CASE WHEN fl > 0.1 THEN 0.3 ELSE 2 END END",
}


def _rounds(tree):
    """Whether the tree has a FLOAT literal that is not its own float."""
    if tree[0] == "lit":
        return "." in tree[1] and C.lit_type(tree[1]) == "FLOAT" and float(np.float32(float(tree[1]))) != float(tree[1])
    return tree[0] != "col" and any(_rounds(a) for a in tree[1])


def test_the_data_tells(data):
    """No GPU work: every WHEN and the ELSE of every query select at least one doc, and wherever a literal is read as a
    float, reading it as a double would change at least one doc's value."""
    t, hs, allc = data
    for name, expr in CASES.items():
        tree = _tree(expr)
        for counts in C.branch_counts(tree, allc):
            assert all(c > 0 for c in counts), (name, counts)
        if _rounds(tree):
            a, b = _docs(allc, tree), C.unrounded_docs(tree, allc)
            assert (np.array([E.canon_bits(v) for v in a.tolist()]) != np.array([E.canon_bits(v) for v in b.tolist()])).any(), name
    d, e = allc["d"], allc["e"]
    eq = _docs(allc, _tree(CASES["zero_signs_and_nans"]))
    assert ((eq == 0) & (d == 0) & (e == 0)).sum() > 0          # -0.0 = 0.0 is false
    assert ((eq == 1) & np.isnan(d) & np.isnan(e)).sum() > 0    # NaN = NaN between two columns is true
    gt = _docs(allc, _tree(CASES["total_order"]))
    assert ((gt == 1) & np.isnan(d) & np.isposinf(e)).sum() > 0  # NaN > everything
    assert (allc["l"] > 2 ** 52).any() and (np.abs(allc["l"]) <= 2 ** 53).all() and (allc["big"] > 2 ** 53).all()


@pytest.mark.parametrize("name", list(CASES))
def test_per_doc_values_are_exact(data, name):
    t, hs, allc = data
    expr = CASES[name]
    q = parse_query("SELECT SUM(%s), MIN(%s), MAX(%s) FROM t GROUP BY id" % (expr, expr, expr))
    r, path, variant = _run(t, hs, q)
    assert variant == DENSE and path == "global"
    vals = _docs(allc, q.expressions[q.aggregations[0][1]]).tolist()
    got = r.as_dict()
    assert len(got) == len(vals) == sum(DOCS)
    for k, v in enumerate(vals):
        s, lo, hi = got[(k,)]
        assert E.canon_bits(lo) == E.canon_bits(hi) == E.canon_bits(v), (k, v, lo, hi)
        assert E.canon_bits(s) == E.canon_bits(0.0 + v)


@pytest.mark.parametrize("f_below", [None, 60], ids=["dense", "sparse"])
@pytest.mark.parametrize("name", ["three_whens", "and", "float_result", "total_order", "case_times"])
def test_parity_in_both_instances(data, name, f_below):
    t, hs, allc = data
    expr = CASES[name]
    where = "" if f_below is None else " WHERE f < %d" % f_below
    mask = np.ones(len(allc["f"]), dtype=bool) if f_below is None else allc["f"] < f_below
    sql = "SELECT SUM(%s), MIN(%s), MAX(%s), AVG(%s), COUNT(%s) FROM t%s GROUP BY g1, g2" % ((expr,) * 5 + (where,))
    r = _check_query(t, hs, allc, sql, mask, path="lds", variant=DENSE if f_below is None else SPARSE)
    # numEntriesScannedPostFilter: every distinct real column of the program once, beside the group-by columns
    ncols = len({"g1", "g2"} | set(expr_columns(_tree(expr))))
    assert r.stats.as_tuple()[2] == int(mask.sum()) * ncols


def test_accumulator_modes_and_aggregation_only(data, oracle):
    t, hs, allc = data
    expr = CASES["float_result"]
    sql = "SELECT SUM(%s), MIN(%s), MAX(%s), MIN(%s), COUNT(*), SUM(q) FROM t WHERE f < %%d GROUP BY g1, g2" \
        % (expr, expr, CASES["and"], CASES["and"])  # six slots of 35 keys: past a 1 KB table
    a = _check_query(t, hs, allc, sql % 500, allc["f"] < 500, path="lds", variant=DENSE).as_dict()
    t.set_config(lds_table_kb=1)  # the same queries on the global table
    try:
        b = _check_query(t, hs, allc, sql % 500, allc["f"] < 500, path="global", variant=DENSE).as_dict()
        _check_query(t, hs, allc, sql % 50, allc["f"] < 50, path="global", variant=SPARSE)
    finally:
        t.reset_config()
    assert repr({k: v[1:] for k, v in a.items()}) == repr({k: v[1:] for k, v in b.items()})  # (repr: a NaN MAX)
    # aggregation only, filtered and not
    for where, m in ((" WHERE f < 300", allc["f"] < 300), ("", np.ones(len(allc["f"]), dtype=bool))):
        q = parse_query("SELECT SUM(%s), MIN(%s), AVG(%s), COUNT(*) FROM t%s"
                        % (CASES["three_whens"], CASES["total_order"], CASES["div_by_zero_unselected"], where))
        _check_query(t, hs, allc, q, m)
        vals = t.execute_aggregation(hs, q).values
        st = E.group_stats([], _docs(allc, _tree(CASES["three_whens"])), m)[()]
        assert vals[0] == st[0] and vals[3] == int(m.sum())  # halves: the sum is exact


def test_hash_key_space(oracle, gpu_lib):
    """9000 x 9000 keys over 9000 docs: past every dense table, so the groups live in the hash table."""
    schema = [("h1", "INT"), ("h2", "INT"), ("v", "INT"), ("w", "DOUBLE")]
    n = 9000
    rng = np.random.default_rng(3)
    cols = {"h1": np.arange(n), "h2": np.arange(n)[::-1].copy(), "v": np.arange(n) % 50 - 20,
            "w": rng.choice([0.1, F01, 0.0, -0.0, 1.5], n)}
    typed = C.typed(cols, schema)
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        expr = "CASE WHEN w > 0.1 THEN v WHEN w = 0.0 THEN 0.1 ELSE w END"
        q = parse_query("SELECT SUM(%s), MIN(%s), COUNT(*) FROM t GROUP BY h1, h2" % (expr, expr), num_groups_limit=10 ** 9)
        r, path, variant = _run(t, [h], q)
        assert path == "hash" and variant == SPARSE
        tree = _tree(expr)
        assert all(c > 0 for c in C.branch_counts(tree, typed)[0])
        vals = C.eval_docs(tree, typed).tolist()
        got = r.as_dict()
        assert len(got) == n
        for k in range(n):
            s, lo, c = got[(k, n - 1 - k)]
            assert (E.bits(s), E.bits(lo), c) == (E.bits(0.0 + vals[k]), E.bits(vals[k]), 1)


def test_order_by_case_aggregation_with_a_trim(data):
    t, hs, allc = data
    expr = CASES["case_times"]
    q = parse_query("SELECT g1, g2, SUM(%s) FROM t WHERE f < 300 GROUP BY g1, g2 ORDER BY SUM(%s) DESC LIMIT 3" % (expr, expr))
    q.min_server_group_trim_size = 1  # the server keeps max(limit * 5, 1) = 15 groups
    top = t.execute_groupby(hs, q).trim_sql()
    st = E.group_stats([allc["g1"], allc["g2"]], _docs(allc, _tree(expr)), allc["f"] < 300)
    order = sorted(st.items(), key=lambda kv: (-kv[1][0], kv[0][1], kv[0][0]))
    assert len(top) == 15
    assert order[2][1][0] - order[3][1][0] > 1e-6 * order[2][1][4]  # (no near-tie at the cut)
    assert top.keys[:3] == [k for k, _ in order[:3]]
    for got, (_, st) in zip(top.values[:3], order[:3]):
        assert abs(got[0] - st[0]) <= TOL * st[4]


def test_reexecution_and_plan_cache(data):
    t, hs, allc = data
    sql = "SELECT SUM(%s), MIN(%s), COUNT(*) FROM t WHERE f %%s 400 GROUP BY g1" % (CASES["three_whens"], CASES["and"])
    q = parse_query(sql % "<")
    with t.plan(hs, q) as p:
        p.execute()
        p.execute()  # the table starts over with every execution: no doubled sums
        twice = p.finalize().as_dict()
    a = _check_query(t, hs, allc, q, allc["f"] < 400).as_dict()
    b = _check_query(t, hs, allc, sql % ">=", allc["f"] >= 400).as_dict()
    c = t.execute_groupby(hs, parse_query(sql % "<")).as_dict()  # a plan-cache hit
    assert repr(twice) == repr(a) == repr(c) and repr(a) != repr(b)  # (repr: a NaN MIN equals itself)


@pytest.mark.parametrize("where, pred", [
    ("CASE WHEN i > 1 THEN x ELSE e END > 1.5", lambda v: v > 1.5),
    ("CASE WHEN d > 0.1 THEN 0.1 ELSE 0.0 END = 0.10000000149011612", lambda v: v == F01),
    ("CASE WHEN d = e THEN 1 ELSE 0 END = 1", lambda v: v == 1),
    ("CASE WHEN i > 0 AND j < 2 THEN q ELSE 0 END / q BETWEEN 0.5 AND 1", lambda v: (v >= 0.5) & (v <= 1)),
])
def test_case_as_a_where_leaf(data, where, pred):
    """The same evaluator in the expression-leaf kernel: the doc set, and numEntriesScannedInFilter as a lone
    expression leaf counts it (tests/test_expr_filter_gpu.py test_alone: every doc)."""
    t, hs, allc = data
    q = parse_query("SELECT COUNT(*), SUM(q) FROM t WHERE %s GROUP BY g1" % where, filter_expressions=True)
    leaf = q.filter.predicate.column
    with np.errstate(invalid="ignore"):
        mask = pred(_docs(allc, q.expressions[leaf]))
    assert 0 < int(mask.sum()) < len(mask)
    r = _check_query(t, hs, allc, q, mask, path="lds")
    assert r.stats.num_entries_scanned_in_filter == sum(DOCS)
    # beside a plain predicate and a CASE aggregation
    q2 = parse_query("SELECT COUNT(*), SUM(%s) FROM t WHERE f < 500 AND %s GROUP BY g1" % (CASES["three_whens"], where),
                     filter_expressions=True)
    _check_query(t, hs, allc, q2, mask & (allc["f"] < 500), path="lds")


def test_long_past_2p53_is_declined_at_plan_time(data):
    t, hs, allc = data
    for sql in ("SELECT SUM(CASE WHEN big > 5 THEN 1 ELSE 0 END) FROM t GROUP BY g1",
                "SELECT SUM(CASE WHEN big = l THEN 1 ELSE 0 END) FROM t GROUP BY g1",
                "SELECT COUNT(*) FROM t WHERE CASE WHEN big > 5 THEN 1 ELSE 0 END = 1 GROUP BY g1"):
        with pytest.raises(L.UnsupportedQueryError) as e:
            t.plan(hs, parse_query(sql, filter_expressions=True))
        assert "expression" in str(e.value) and "2^53" in str(e.value)
    # not compared as it is: the value is what SUM(big - i) has always read
    for sql in ("SELECT MAX(CASE WHEN i > 0 THEN big ELSE 0 END) FROM t GROUP BY g1",
                "SELECT MAX(CASE WHEN big - l > 5 THEN 1 ELSE 0 END) FROM t GROUP BY g1"):
        _check_query(t, hs, allc, sql, np.ones(len(allc["f"]), dtype=bool), variant=DENSE)
    with pytest.raises(ValueError):  # the Python layer's own decline: a LONG against a FLOAT / DOUBLE side
        t.plan(hs, parse_query("SELECT SUM(CASE WHEN l > 0.5 THEN 1 ELSE 0 END) FROM t GROUP BY g1"))


def test_registration_type_check(data):
    """pgpu_table_add_expression: EXPR_BAD_TYPE, the new ops' names, and the ops that stay unknown."""
    t, hs, allc = data
    i, j = t.index["i"], t.index["j"]
    Cc, Lt = L.EXPR_COLUMN, L.EXPR_LITERAL
    bad = [([(Cc, i, 0), (Cc, j, 0), (L.EXPR_GT, 0, 0), (Cc, i, 0), (L.EXPR_GT, 0, 0)], "bad operand type"),      # CMP on a boolean
           ([(Cc, i, 0), (Cc, j, 0), (Cc, i, 0), (L.EXPR_SELECT, 0, 0)], "bad operand type"),                      # no boolean on top
           ([(Cc, i, 0), (Cc, j, 0), (L.EXPR_GT, 0, 0)], "bad operand type"),                                      # leaves a boolean
           ([(Cc, i, 0), (Cc, j, 0), (L.EXPR_AND, 0, 0)], "bad operand type"),
           ([(Cc, i, 0), (Cc, j, 0), (L.EXPR_GT, 0, 0), (L.EXPR_SELECT, 0, 0)], "underflow"),
           ([(Cc, i, 0), (Cc, j, 0), (15, 0, 0)], "unknown op"),
           ([(Cc, i, 0), (Cc, j, 0), (Cc, i, 0), (Cc, j, 0), (L.EXPR_GT, 0, 0), (Cc, j, 0), (Cc, i, 0)], "deeper")]  # AND needs 5
    for ops, word in bad:
        with pytest.raises(L.PinotGpuError) as e:
            t.add_expression(ops)
        assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and word in str(e.value), str(e.value)
    col = t.add_expression([(Lt, 0, 0.5), (Cc, i, 0), (Cc, i, 0), (Cc, j, 0), (L.EXPR_LE, 0, 0), (L.EXPR_SELECT, 0, 0)])
    assert t.expression(col)[1] == "case(less_than_or_equal(i,j),i,0.5)"


def test_one_rank_host_communicator(data):
    from pinot_amd.combine import Communicator, combine_mode, combine_plan
    t, hs, allc = data
    q = parse_query("SELECT COUNT(*), SUM(%s), MIN(%s), MAX(%s) FROM t WHERE f < 500 GROUP BY g1, g2"
                    % (CASES["three_whens"], CASES["total_order"], CASES["and"]))
    want = _check_query(t, hs, allc, q, allc["f"] < 500).as_dict()
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
        assert got[k][:2] == want[k][:2]  # (sums of halves are order-independent)
        assert [E.canon_bits(v) for v in got[k][2:]] == [E.canon_bits(v) for v in want[k][2:]]
