"""Expressions in GROUP BY on the GPU: the derived column of a group-by expression -- a dictionary and a fixed-bit
forward index per pinned segment, built on the GPU on first use -- and the queries that group by it.  The yardstick is
numpy over case_common.eval_docs (the reference's typing rules restated; it never calls the compiler or the library
under test): the per-doc doubles, read as the expression's result type R and grouped by their bits in the dictionaries'
order (-0.0 and +0.0 apart, every NaN one group).  Integer and COUNT answers are exact; double sums within the project's
1e-9 relative to the sum of |terms|.  Shapes as in test_case_expr_gpu.py, for its reasons: segments of 8192 + 37 docs (a
whole tile and a tail), 100 docs (a lane tail) and one doc.  Every test fails without the feature: the parser flag
and the ABI call do not exist there."""
import numpy as np
import pytest

import case_common as C
import expr_common as E
import percentile_common as P
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import expr_columns, parse_query
from pinot_amd.segment import SegmentBuffers

pytestmark = pytest.mark.gpu
SPARSE, DENSE = 12, 13
TOL = 1e-9

# test_case_expr_gpu.py's kind of schema: id is unique over the segments; f selects; i, j are small INTs (so i * j holds
# -0.0 and +0.0); l is a LONG within +-2^53, big a LONG past it; fl a FLOAT; d and e DOUBLEs holding -0.0, +0.0, NaN,
# +-inf; x a full-mantissa DOUBLE; q a positive INT.
SCHEMA = [("g1", "INT"), ("g2", "INT"), ("id", "INT"), ("f", "INT"), ("i", "INT"), ("j", "INT"), ("l", "LONG"),
          ("big", "LONG"), ("fl", "FLOAT"), ("d", "DOUBLE"), ("e", "DOUBLE"), ("x", "DOUBLE"), ("q", "INT")]
DOCS = (8192 + 37, 100, 1)
F01 = float(np.float32(0.1))
SPECIAL = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.1, F01, 1.0, -1.0, 2.5, 1e300, -1e-300]
FLOATS = [0.1, float(np.nextafter(np.float32(0.1), np.float32(1))), 0.3, -2.5, 0.0, 2.5]
TYPE_CODE = {"INT": L.INT, "LONG": L.LONG, "FLOAT": L.FLOAT, "DOUBLE": L.DOUBLE}


def _columns(rng, n, id0):
    return {"g1": rng.integers(0, 7, n), "g2": rng.integers(10, 15, n), "id": np.arange(id0, id0 + n),
            "f": rng.integers(0, 1000, n), "i": rng.integers(-3, 4, n), "j": rng.integers(-3, 4, n),
            "l": rng.integers(0, 300, n).astype(np.int64) + (rng.random(n) < 0.05) * (1 << 52),
            "big": (1 << 60) + rng.integers(0, 4000, n).astype(np.int64) * 3 + 1,
            "fl": rng.choice(FLOATS, n).astype(np.float32), "d": rng.choice(SPECIAL, n), "e": rng.choice(SPECIAL, n),
            "x": rng.uniform(1.0, 2.0, n), "q": rng.integers(1, 9, n)}


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(47)
    cols, id0 = [], 0
    for n in DOCS:
        cols.append(_columns(rng, n, id0))
        id0 += n
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(oracle.make_segment(SCHEMA, c)) for c in cols]
    segc = [C.typed(c, SCHEMA) for c in cols]
    allc = C.typed({name: np.concatenate([c[name] for c in cols]) for name, _ in SCHEMA}, SCHEMA)
    yield t, hs, segc, allc
    t.close()


def _q(sql, **kw):
    return parse_query(sql, filter_expressions=True, group_by_expressions=True, **kw)


_DOC_CACHE = {}


def _docs(cols, tree):
    """The yardstick's per-doc doubles of a tree over typed columns, computed once per (expression, column set)."""
    k = (repr(tree), id(cols))
    if k not in _DOC_CACHE:
        _DOC_CACHE[k] = (cols, C.eval_docs(tree, cols))  # (cols kept: its id stays its own)
    return _DOC_CACHE[k][1]


def _typed_values(tree, cols):
    """(R, the per-doc values as R holds them): int64 for INT / LONG, the doubles for FLOAT / DOUBLE (a FLOAT-typed CASE
    yields (double)(float) values by construction, which the test asserts)."""
    r = C.node_type(tree, cols)
    v = _docs(cols, tree)
    if r in ("INT", "LONG"):
        assert np.all(v == np.floor(v)) and np.all(np.abs(v) <= 2.0 ** 53)
        return r, v.astype(np.int64)
    if r == "FLOAT":
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v, equal_nan=True)
    return r, v


def _canon(x):
    """A key's identity: an integer as it is, a double by its bits (every NaN the canonical one)."""
    return int(x) if isinstance(x, (int, np.integer)) else E.canon_bits(x)


def _key_arrays(q, cols):
    """Per group-by entry the per-doc key identities (Python ints, in object arrays: bit patterns go up to 2^64)."""
    out = []
    for c in q.group_by:
        if c in q.expressions:
            r, v = _typed_values(q.expressions[c], cols)
            ids = [_canon(x) for x in v.tolist()]
        else:
            ids = [int(x) for x in cols[c].tolist()]
        a = np.empty(len(ids), dtype=object)
        a[:] = ids
        out.append(a)
    return out


def _projected(q):
    """The distinct real columns the query projects: group-by columns and operands, aggregation columns and operands."""
    cols = set()
    for c in q.group_by + [c for _, c in q.aggregations if c != "*"]:
        cols |= set(expr_columns(q.expressions[c])) if c in q.expressions else {c}
    return cols


def _run(t, hs, q):
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        return r, p.group_path(), p.scan_geometry()["variant"]


def _got(r):
    """{key identities: row}; the groups must be distinct under the identity (0.0 and -0.0 are, two NaNs are not)."""
    out = {tuple(_canon(x) for x in k): v for k, v in zip(r.keys, r.values)}
    assert len(out) == len(r)
    return out


def _check_agg(fn, got, st, whole):
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
        if not np.isfinite(s) or (whole and mag < 2.0 ** 53):
            assert E.canon_bits(got) == E.canon_bits(s)
        else:
            assert abs(got - s) <= TOL * mag, (got, s, mag)


def _check_query(t, hs, allc, sql, mask=None, path=None, variant=None, **kw):
    """Runs the query and compares groups, COUNT / SUM / MIN / MAX / AVG values and the two scan statistics with the
    yardstick.  DISTINCTCOUNT and PERCENTILE columns are checked by the caller."""
    q = _q(sql, **kw) if isinstance(sql, str) else sql
    mask = np.ones(len(allc["f"]), dtype=bool) if mask is None else np.asarray(mask)
    r, gpath, gvariant = _run(t, hs, q)
    if path:
        assert gpath == path
    if variant is not None:
        assert gvariant == variant
    got = _got(r)
    keys = _key_arrays(q, allc)
    stats = {}
    for fn, col in q.aggregations:
        if col in stats or fn == "DISTINCTCOUNT" or fn.startswith("PERCENTILE"):
            continue
        vals = np.zeros(len(mask)) if col == "*" else \
            _docs(allc, q.expressions[col]) if col in q.expressions else allc[col].astype(np.float64)
        with np.errstate(invalid="ignore"):
            whole = bool(np.all(vals[mask] == np.floor(vals[mask])))
        stats[col] = (E.group_stats(keys, vals, mask), whole)
    want = next(iter(stats.values()))[0]
    assert set(got) == set(want)
    for k, row in got.items():
        for (fn, col), v in zip(q.aggregations, row):
            if col in stats:
                _check_agg(fn, v, stats[col][0][k], stats[col][1])
    assert r.stats.num_docs_scanned == int(mask.sum())
    assert r.stats.num_entries_scanned_post_filter == int(mask.sum()) * len(_projected(q))
    return r, q


# ------------------------------------------------------------------------------------------------ 1. bytes
# name -> (expression, R, derived cardinality in the 8229-doc segment)
BYTES = {
    "card1": ("i * 0 + 1", "DOUBLE", 1),
    "card2": ("CASE WHEN i > 0 THEN 1 ELSE 0 END", "INT", 2),
    "card3": ("CASE WHEN i < -1 THEN 0 WHEN i < 2 THEN 1 ELSE 2 END", "INT", 3),
    "card7_long": ("CASE WHEN i > 100 THEN l ELSE i END", "LONG", 7),
    "card49": ("i * 10 + j", "DOUBLE", 49),
    "float": ("CASE WHEN q > 4 THEN fl ELSE 0.5 END", "FLOAT", 7),
    "wide": ("id + 1", "DOUBLE", 8192 + 37),
}


@pytest.mark.parametrize("name", list(BYTES))
def test_derived_column_bytes(data, oracle, name):
    """The derived column is, byte for byte, the dictionary and forward index the segment creator writes for a column of
    type R holding the yardstick's per-doc values: in every segment size, and the tail docs read back one by one."""
    t, hs, segc, allc = data
    expr, rtype, card0 = BYTES[name]
    q = _q("SELECT COUNT(*) FROM t GROUP BY %s" % expr)
    gname = q.group_by[0]
    t.query_c(q)  # registers the expression: nothing is built yet
    assert t.index[("group", gname)] >= L.GROUP_EXPR_COLUMN_BASE and t.group_types[gname] == TYPE_CODE[rtype]
    bits_seen = []
    for h, cols in zip(hs, segc):
        r, vals = _typed_values(q.expressions[gname], cols)
        assert r == rtype
        want = oracle.build_column(TYPE_CODE[rtype], vals)
        card, bits, dict_bytes, fwd_bytes = t.segment_column_bytes(h, ("group", gname))
        assert (card, bits) == (want.cardinality, want.bits_per_element)
        assert dict_bytes == want.dict_bytes
        assert fwd_bytes == want.fwd_bytes
        bits_seen.append(bits)
        n = len(vals)
        docs = np.arange(max(0, n - 70), n)
        dtype = {"INT": ">i4", "LONG": ">i8", "FLOAT": ">f4", "DOUBLE": ">f8"}[rtype]
        dvals = np.frombuffer(dict_bytes, dtype=dtype)
        ids = t.read_dict_ids(h, ("group", gname), docs)
        assert np.array_equal(dvals[ids].astype(np.float64), np.asarray(vals[docs], dtype=np.float64))
    assert bits_seen[0] == max(1, int(card0 - 1).bit_length()) and bits_seen[2] == 1
    assert _got_card(t, hs[0], gname) == card0


def _got_card(t, h, gname):
    return t.segment_column_bytes(h, ("group", gname))[0]


def test_table_dictionary_of_a_derived_column(data):
    t, hs, segc, allc = data
    q = _q("SELECT COUNT(*) FROM t GROUP BY CASE WHEN i < -1 THEN 0 WHEN i < 2 THEN 1 ELSE 2 END, d / e")
    t.query_c(q)
    assert t.dictionary(("group", q.group_by[0])) == [0, 1, 2]
    vals = _docs(allc, q.expressions[q.group_by[1]])
    want = sorted({E.key(v) for v in vals.tolist()})
    got = t.dictionary(("group", q.group_by[1]))
    assert [E.key(v) for v in got] == want  # ascending in the dictionaries' order, NaN on top, each value once
    assert np.isnan(got[-1]) and got[-2] == float("inf")


# ------------------------------------------------------------------------------------------------ 2. queries
def test_int_case_buckets(data):
    t, hs, segc, allc = data
    r, q = _check_query(t, hs, allc, "SELECT COUNT(*), SUM(q), MIN(x), MAX(l) FROM t "
                        "GROUP BY CASE WHEN i < -1 THEN 0 WHEN i < 2 THEN 1 ELSE 2 END", path="lds")
    assert sorted(r.keys) == [(0,), (1,), (2,)] and all(isinstance(k[0], int) for k in r.keys)


def test_product_with_signed_zeros(data):
    t, hs, segc, allc = data
    r, q = _check_query(t, hs, allc, "SELECT i * j, COUNT(*), SUM(x) FROM t GROUP BY i * j", path="lds")
    zeros = [k[0] for k in r.keys if k[0] == 0.0]
    assert sorted(np.signbit(z) for z in zeros) == [False, True]  # -0.0 and +0.0 are two groups
    assert all(isinstance(k[0], float) for k in r.keys)


def test_quotient_with_nan_inf_and_zeros(data):
    t, hs, segc, allc = data
    r, q = _check_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t GROUP BY d / e", path="lds")
    ks = [k[0] for k in r.keys]
    assert sum(np.isnan(k) for k in ks) == 1 and float("inf") in ks and float("-inf") in ks
    assert sorted(np.signbit(k) for k in ks if k == 0.0) == [False, True]


def test_float_typed_case(data):
    t, hs, segc, allc = data
    r, q = _check_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t GROUP BY CASE WHEN d > 0.1 THEN fl ELSE 0.5 END",
                        path="lds")
    assert C.node_type(q.expressions[q.group_by[0]], allc) == "FLOAT"
    assert F01 in [k[0] for k in r.keys] and 0.1 not in [k[0] for k in r.keys]  # the FLOAT's double, not the literal's


def test_beside_a_plain_column_and_two_expressions(data):
    t, hs, segc, allc = data
    _check_query(t, hs, allc, "SELECT g1, i + j, COUNT(*), SUM(x), AVG(q) FROM t GROUP BY g1, i + j", path="lds")
    # two expressions, one of them of 8330 values: 17 x 8330 keys are past the LDS table
    # (numGroupsLimit above the key space: below it the plan is split per segment, test_num_groups_limit_*)
    r, q = _check_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t GROUP BY i * j, id + 1", path="global",
                        num_groups_limit=10 ** 9)
    assert len(r) == sum(DOCS)
    _check_query(t, hs, allc, "SELECT COUNT(*), MAX(x) FROM t GROUP BY id + 1, g2", path="global")


def test_with_filters(data):
    t, hs, segc, allc = data
    _check_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t WHERE f < 300 GROUP BY i * j, g1", allc["f"] < 300,
                 path="lds")
    with np.errstate(invalid="ignore"):
        m = (_docs(allc, _q("SELECT SUM(x * q) FROM t").expressions["mult(x,q)"]) > 6) & (allc["f"] >= 100)
    assert 0 < m.sum() < len(m)
    r, q = _check_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t WHERE x * q > 6 AND f >= 100 "
                        "GROUP BY CASE WHEN i < -1 THEN 0 WHEN i < 2 THEN 1 ELSE 2 END, id + 1", m, path="global")
    assert r.stats.num_entries_scanned_in_filter > 0


def test_beside_an_expression_aggregation(data):
    t, hs, segc, allc = data
    sql = "SELECT COUNT(*), SUM(x * q), MAX(x * q), SUM(i * j) FROM t%s GROUP BY i * j, g2"
    _check_query(t, hs, allc, sql % "", path="lds", variant=DENSE)
    _check_query(t, hs, allc, sql % " WHERE f < 100", allc["f"] < 100, path="lds", variant=SPARSE)
    _check_query(t, hs, allc, "SELECT COUNT(*), SUM(x * q) FROM t GROUP BY id + 1", path="global", variant=DENSE)
    _check_query(t, hs, allc, "SELECT COUNT(*), SUM(x * q) FROM t WHERE f < 100 GROUP BY id + 1", allc["f"] < 100,
                 path="global", variant=SPARSE)


def test_beside_distinctcount_and_percentile(data):
    t, hs, segc, allc = data
    for sql in ("SELECT COUNT(*), DISTINCTCOUNT(g2), SUM(q) FROM t WHERE f < 700 GROUP BY i * j",
                "SELECT COUNT(*), PERCENTILE50(q), DISTINCTCOUNT(g2) FROM t WHERE f < 700 GROUP BY i * j"):
        m = allc["f"] < 700
        r, q = _check_query(t, hs, allc, sql, m, path="lds")
        keys = _key_arrays(q, allc)[0]
        pct = P.percentiles([keys], allc["q"], m, 50)
        for k, row in _got(r).items():
            for (fn, col), v in zip(q.aggregations, row):
                if fn == "DISTINCTCOUNT":
                    assert v == len(set(allc[col][m & (keys == k[0])].tolist()))
                elif fn.startswith("PERCENTILE"):
                    assert v == pct[k]


def test_order_by_the_expression_with_limit(data):
    t, hs, segc, allc = data
    q = _q("SELECT i * j, COUNT(*) FROM t GROUP BY i * j ORDER BY i * j DESC LIMIT 3")
    q.min_server_group_trim_size = 1  # the server keeps max(limit * 5, 1) = 15 groups, in ORDER BY order
    top = t.execute_groupby(hs, q).trim_sql()
    vals = _docs(allc, q.expressions["mult(i,j)"])
    order = sorted({E.key(v) for v in vals.tolist()}, reverse=True)
    assert [E.key(k[0]) for k in top.keys[:3]] == order[:3]
    for k, v in zip(top.keys[:3], top.values[:3]):
        assert v[0] == int((vals == k[0]).sum())
    q = _q("SELECT g1, COUNT(*) FROM t GROUP BY g1, CASE WHEN i > 0 THEN 1 ELSE 0 END "
           "ORDER BY CASE WHEN i > 0 THEN 1 ELSE 0 END, g1 DESC LIMIT 4")
    q.min_server_group_trim_size = 1
    top = t.execute_groupby(hs, q).trim_sql()
    assert top.keys[:4] == [(6, 0), (5, 0), (4, 0), (3, 0)]


def test_names_in_string_keys_and_the_datatable(data):
    t, hs, segc, allc = data
    q = _q("SELECT COUNT(*) FROM t GROUP BY g1, CASE WHEN i > 0 THEN 1 ELSE 0 END, i * j")
    r = t.execute_groupby(hs, q)
    sk = r.string_keys()
    assert len(sk) == len(r)
    keys = _key_arrays(q, allc)
    vals = _docs(allc, q.expressions["mult(i,j)"]).tolist()
    want = {"\0".join([str(a), str(b), repr(v)]) for a, b, v in zip(keys[0].tolist(), keys[1].tolist(), vals)}  # "3\x001\x00-0.0"
    assert set(sk) == want
    table = r.datatable()  # the server's response: values travel, and the key columns are named by the function form
    assert b"case(greater_than(i,0),1,0)" in table and b"mult(i,j)" in table


# ------------------------------------------------------------------------------------------------ 3. numGroupsLimit
def test_num_groups_limit_keeps_the_first_seen_groups(data):
    t, hs, segc, allc = data
    cols = segc[0]
    q = _q("SELECT COUNT(*), SUM(q) FROM t GROUP BY i * j", num_groups_limit=3)
    keys = _key_arrays(q, cols)[0]
    first = list(dict.fromkeys(keys.tolist()))[:3]  # the first three distinct values in doc order
    r = t.execute_groupby([hs[0]], q)
    got = _got(r)
    assert set(got) == {(k,) for k in first}
    for k in first:
        sel = keys == k
        assert got[(k,)] == [int(sel.sum()), float(cols["q"][sel].sum())]


# ------------------------------------------------------------------------------------------------ 4. growth
def test_a_later_segment_grows_the_derived_dictionary(oracle, gpu_lib):
    schema = [("g", "INT"), ("i", "INT"), ("j", "INT")]
    rng = np.random.default_rng(9)
    a = {"g": rng.integers(0, 3, 300), "i": rng.integers(0, 3, 300), "j": rng.integers(1, 3, 300)}
    b = {"g": rng.integers(0, 3, 8192 + 5), "i": rng.integers(-5, 6, 8192 + 5), "j": rng.integers(1, 7, 8192 + 5)}
    sql = "SELECT COUNT(*), SUM(g) FROM t GROUP BY i * j"
    with GpuTable(schema) as t:
        empty = t.device_bytes()
        ha = t.pin_segment(oracle.make_segment(schema, a))
        pinned = t.device_bytes()
        ta = C.typed(a, schema)
        r1, q = _check_query(t, [ha], {**ta, "f": ta["g"]}, sql, path="lds")
        first = _got(r1)
        undecoded = t.execute_groupby([ha], q)  # its keys are read after the dictionary has grown
        card, bits, _, _ = t.segment_column_bytes(ha, ("group", "mult(i,j)"))
        assert t.device_bytes() >= pinned + ((300 + 8191) // 8192 * 256 * bits + 4) * 4  # the derived forward index
        hb = t.pin_segment(oracle.make_segment(schema, b))
        both = C.typed({k: np.concatenate([a[k], b[k]]) for k in a}, schema)
        r2, _ = _check_query(t, [ha, hb], {**both, "f": both["g"]}, sql, path="lds")
        assert len(r2) > len(r1) and set(first) < set(_got(r2))
        assert _got(undecoded) == first  # the first plan's result keeps its labels: it reads the snapshot it was planned on
        assert len(t.dictionary(("group", "mult(i,j)"))) == len(r2)
        t.unpin_segment(ha)
        t.unpin_segment(hb)
        assert t.device_bytes() == empty  # the derived columns' bytes went with their segments


# ------------------------------------------------------------------------------------------------ 5. declines
def _declined(fn, *words):
    with pytest.raises(L.UnsupportedQueryError) as e:
        fn()
    assert "GROUP BY expression" in str(e.value), str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_operand_product_cap(oracle, gpu_lib):
    schema = [("a", "INT"), ("b", "INT"), ("c", "INT"), ("e", "INT")]
    n = 8192 + 37
    k = np.arange(n)
    cols = {"a": k % 2100, "b": (k * 11) % 2100, "c": k % 2048, "e": (k // 4) % 2048}
    assert len(set(cols["b"].tolist())) == 2100 and len(set(cols["e"].tolist())) == 2048
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        _declined(lambda: t.plan([h], _q("SELECT COUNT(*) FROM t GROUP BY a + b")), "combinations")  # 4 410 000 > 2^22
        tc = C.typed(cols, schema)
        _check_query(t, [h], {**tc, "f": tc["a"]}, "SELECT COUNT(*), SUM(a) FROM t GROUP BY c * 4096 + e")  # 2^22 exactly


def test_declined_operands(data, oracle):
    from pinot_amd.segment import build_raw_column
    t, hs, segc, allc = data
    # R = LONG over a LONG column past +-2^53; the same column compared as it is
    _declined(lambda: t.plan(hs, _q("SELECT COUNT(*) FROM t GROUP BY CASE WHEN i > 0 THEN big ELSE 0 END")), "2^53")
    _declined(lambda: t.plan(hs, _q("SELECT COUNT(*) FROM t GROUP BY CASE WHEN big > 5 THEN 1 ELSE 0 END")), "2^53")
    _check_query(t, hs, allc, "SELECT COUNT(*) FROM t GROUP BY CASE WHEN i > 0 THEN l ELSE 0 END")  # within: runs
    schema = [("g", "INT"), ("s", "STRING"), ("v", "INT"), ("w", "LONG")]
    n = 64
    base = oracle.make_segment(schema[:3], {"g": np.arange(n) % 4, "s": ["k%d" % (k % 5) for k in range(n)],
                                            "v": np.arange(n)})
    cols = {**base.columns, "w": build_raw_column("LONG", (np.arange(n, dtype=np.int64) * 3).tolist(), 2)}
    with GpuTable(schema) as t2:
        h = t2.pin_segment(SegmentBuffers(n, cols))
        _declined(lambda: t2.plan([h], _q("SELECT COUNT(*) FROM t GROUP BY s + 1")), "STRING")  # at registration
        _declined(lambda: t2.plan([h], _q("SELECT COUNT(*) FROM t GROUP BY v * w")), "raw")
        r = t2.execute_groupby([h], _q("SELECT COUNT(*), SUM(w) FROM t GROUP BY v * 2"))  # a raw column beside it runs
        assert len(r) == n and sum(v[0] for v in r.values) == n


def test_index_rules(data):
    """A derived column's index is for group_by alone; an aggregation's virtual column stays no group-by column."""
    t, hs, segc, allc = data
    q = _q("SELECT COUNT(*), SUM(q) FROM t WHERE f < 500 GROUP BY i * j")
    t.query_c(q)
    derived = t.index[("group", "mult(i,j)")]
    assert derived >= L.GROUP_EXPR_COLUMN_BASE
    ops, _ = t._expr_ops(q.expressions["mult(i,j)"])  # the program as the Python layer registers it: 1.0 * i * j
    assert t.add_group_expression(ops, "DOUBLE") == derived          # the identity is (program, result type)
    assert t.add_group_expression(ops, "LONG") not in (derived, t.add_expression(ops))
    virtual = t.add_expression(ops)
    assert len(SCHEMA) <= virtual < L.GROUP_EXPR_COLUMN_BASE
    to_c = q.to_c

    def predicate_on_derived(index):
        c, keep = to_c(index)
        c.predicates[0].column = derived
        return c, keep

    def aggregation_on_derived(index):
        c, keep = to_c(index)
        c.aggs[1].column = derived
        return c, keep

    def group_by_virtual(index):
        c, keep = to_c(index)
        c.group_by[0] = virtual
        return c, keep

    def group_by_unregistered(index):
        c, keep = to_c(index)
        c.group_by[0] = L.GROUP_EXPR_COLUMN_BASE + L.GROUP_EXPR_MAX_PER_TABLE - 1
        return c, keep

    try:
        for bad in (predicate_on_derived, aggregation_on_derived, group_by_virtual, group_by_unregistered):
            q.to_c = bad
            q.__dict__.pop("_c_cache", None)
            with pytest.raises(L.PinotGpuError) as e:
                t.plan(hs, q)
            assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and "bad column" in str(e.value), (bad.__name__, str(e.value))
    finally:
        del q.to_c
        q.__dict__.pop("_c_cache", None)
    with pytest.raises(L.PinotGpuError) as e:
        t.add_group_expression(ops, 4)  # STRING is no result type
    assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT


def test_declined_external_merges(data):
    """finalize_range, an external d_table (execute, finalize, create_execute), exchange_counts, and combine_mode /
    combine on a one-rank host communicator decline; the DataTable, which carries values, is made."""
    import torch
    from pinot_amd.combine import Communicator, combine_mode, combine_plan
    t, hs, segc, allc = data
    q = _q("SELECT COUNT(*), SUM(q) FROM t GROUP BY g1, i * j")
    d = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    _declined(lambda: t.plan_execute(hs, q, d_table=d.data_ptr()))
    comm = Communicator(L.COMM_HOST, Communicator.unique_id(L.COMM_HOST), 1, 0, 0)
    try:
        with t.plan(hs, q) as p:
            ns, nk, kinds = p.layout()
            _declined(lambda: p.execute(None, d.data_ptr()))
            p.execute()
            _declined(lambda: p.finalize(None, d.data_ptr()))
            _declined(lambda: p.finalize_range(None, d.data_ptr(), 0, nk))
            _declined(lambda: p.exchange_counts(None, 2))
            _declined(lambda: combine_mode(p, comm, 1 << 62))
            _declined(lambda: combine_plan(p, comm, None, 0))
            r = p.finalize()
            assert len(r.datatable()) > 0
    finally:
        comm.close()
