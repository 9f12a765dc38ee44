"""Math and time functions in expressions on the GPU: ABS / CEIL / FLOOR / SQRT / MOD and the long arithmetic of
TIMECONVERT / DATETIMECONVERT inside aggregations (both scan instances, the LDS and the global table), in GROUP BY (derived
LONG columns) and in WHERE (expression leaves).  The yardstick is typed numpy written out per expression in this file --
np.fmod for %, truncation toward zero for the long division (time_common.np_tdiv), int64 arithmetic for the time
functions -- and never the library's own lowering.  The column values are chosen so that every asserted sum is exactly
representable (integers and quarters far below 2^53; infinities and NaN are order-independent), so every comparison is bit
for bit; the one family of inexact values, the square roots of imperfect squares, is summed one doc per group.  Shapes
as in test_group_expr_gpu.py: segments of 8192 + 37 docs, 100 docs and one doc.  Every test fails without the feature:
the parser raises `unknown function`, and the library answers `unknown op` to the new codes."""
import numpy as np
import pytest

import expr_common as E
import test_expr_filter_cpu as M
import time_common as T
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import parse_query

pytestmark = pytest.mark.gpu
SPARSE, DENSE = 12, 13
DAY, HOUR, MIN15, WEEK = 86400000, 3600000, 900000, 604800000
DAY0 = 1505865600000  # 2017-09-20T00:00:00Z, in milliseconds

# g1: 7 groups (the LDS table); country: 5; id: unique (the global table, one doc per group); f selects; l: a LONG with
# negatives, 0, values at and one off the bucket boundaries of 10, 7 and a day, and +-2^53 and +-(2^53 - 1), the extremes
# the range check admits; ts: milliseconds within the first five hours of one day; d: a DOUBLE with +-0.0, halves of both
# signs, +-inf, NaN, perfect and imperfect squares; q: a small positive INT.
SCHEMA = [("g1", "INT"), ("country", "INT"), ("id", "INT"), ("f", "INT"), ("l", "LONG"), ("ts", "LONG"), ("d", "DOUBLE"),
          ("q", "INT")]
DOCS = (8192 + 37, 100, 1)
L_EDGES = [-1, 0, 1, 9, 10, 11, -9, -10, -11, 6, 7, 8, -6, -7, -8, DAY - 1, DAY, DAY + 1, -DAY + 1, -DAY, -DAY - 1,
           17428 * DAY, 17428 * DAY - 1, 2 ** 53, -2 ** 53, 2 ** 53 - 1, -(2 ** 53 - 1)]
D_VALUES = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, float("inf"), float("-inf"), float("nan"), 4.0, 9.0, 2.25, 6.25,
            2.0, 3.0, 10.0, -4.0, -2.0, 7.5, 1024.0]


def _columns(rng, n, id0):
    l = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    l[:min(n, len(L_EDGES))] = L_EDGES[:n]
    d = rng.choice([v for v in D_VALUES if np.isfinite(v)], n)  # (the infinities and NaN a few times: most sums stay finite)
    d[:min(n, len(D_VALUES))] = D_VALUES[:n]
    return {"g1": rng.integers(0, 7, n), "country": rng.integers(0, 5, n), "id": np.arange(id0, id0 + n),
            "f": rng.integers(0, 1000, n), "l": l, "ts": DAY0 + rng.integers(0, 300 * 60000, n).astype(np.int64), "d": d,
            "q": rng.integers(1, 9, n)}


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(53)
    cols, id0 = [], 0
    for n in DOCS:
        cols.append(_columns(rng, n, id0))
        id0 += n
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(oracle.make_segment(SCHEMA, c)) for c in cols]
    allc = {name: np.concatenate([c[name] for c in cols]) for name, _ in SCHEMA}
    yield t, hs, cols, allc
    t.close()


def _q(sql, **kw):
    return parse_query(sql, filter_expressions=True, group_by_expressions=True, **kw)


def _f(a):
    return np.asarray(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the known answers
def _kat_cases():
    kat = T.load_kat()
    out = [("dateTimeConvert(ts,'%s','%s','%s')" % (c["in"], c["out"], c["granularity"]), c) for c in kat["datetimeconvert"]]
    return out + [("timeConvert(ts,'%s','%s')" % (c["in"], c["out"]), c) for c in kat["timeconvert"]]


@pytest.mark.parametrize("expr, case", _kat_cases(), ids=[c["name"] for _, c in _kat_cases()])
def test_known_answers_end_to_end(oracle, gpu_lib, expr, case):
    """A table whose docs are the fixture's inputs: the buckets as LONG group keys with their counts, and MIN / MAX of
    the function per doc as doubles."""
    schema = [("id", "INT"), ("ts", "LONG")]
    inp, exp = case["input"], case["expected"]
    cols = {"id": np.arange(len(inp)), "ts": np.asarray(inp, dtype=np.int64)}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        r = t.execute_groupby([h], _q("SELECT COUNT(*) FROM t GROUP BY %s" % expr))
        want = {}
        for v in exp:
            want[(v,)] = [want.get((v,), [0])[0] + 1]
        assert r.as_dict() == want
        assert all(type(k[0]) is int for k in r.keys)
        r = t.execute_groupby([h], _q("SELECT MAX(%s), MIN(%s) FROM t GROUP BY id" % (expr, expr)))
        assert r.as_dict() == {(i,): [float(v), float(v)] for i, v in enumerate(exp)}
        a = t.execute_aggregation([h], _q("SELECT MAX(%s), MIN(%s) FROM t" % (expr, expr)))
        assert a.values == [float(max(exp)), float(min(exp))]


# ------------------------------------------------------------------------------------------------ 2. the ops per doc
def _case_mod(c):
    m = np.fmod(_f(c["l"]), 2.0)
    return np.where(E_KEYS(m) == E_KEYS(np.zeros(len(m))), _f(c["q"]), 0.0)


def E_KEYS(v):
    """Double.doubleToLongBits of each value: -0.0 is not +0.0 (the comparison inside a CASE is Double.compare)."""
    b = np.asarray(v, dtype=np.float64).view(np.uint64).copy()
    b[np.isnan(v)] = E.NAN_KEY
    return b


# name -> (SQL, yardstick over the typed columns, sums exact under GROUP BY g1)
OPS = {
    "abs": ("abs(d)", lambda c: np.abs(c["d"]), True),
    "ceil": ("ceil(d)", lambda c: np.ceil(c["d"]), True),
    "floor": ("floor(d)", lambda c: np.floor(c["d"]), True),
    "sqrt": ("sqrt(d)", lambda c: np.sqrt(c["d"]), False),
    "mod_d_3": ("mod(d, 3)", lambda c: np.fmod(c["d"], 3.0), True),
    "mod_l_minus7": ("mod(l, -7)", lambda c: np.fmod(_f(c["l"]), -7.0), True),
    "floor_l_10": ("floor(l / 10)", lambda c: np.floor(_f(c["l"]) / 10.0), True),
    "days": ("timeconvert(l,'MILLISECONDS','DAYS')", lambda c: _f(T.np_tdiv(c["l"], DAY)), True),
    "case_mod": ("CASE WHEN mod(l, 2) = 0 THEN q ELSE 0 END", _case_mod, True),
    "nested": ("q * floor(sqrt(abs(d)))", lambda c: 1.0 * _f(c["q"]) * np.floor(np.sqrt(np.abs(c["d"]))), True),
}


def _check_agg(fn, got, st, exact):
    s, lo, hi, cnt, mag = st
    if fn == "COUNT":
        assert got == cnt
    elif fn == "MIN":
        assert E.canon_bits(got) == E.canon_bits(lo)
    elif fn == "MAX":
        assert E.canon_bits(got) == E.canon_bits(hi)
    elif exact:
        if fn == "AVG":
            assert got.count == cnt
            got = got.sum
        assert E.canon_bits(got) == E.canon_bits(s), (fn, got, s)


def _run_ops(t, hs, allc, name, group, where, variant, path):
    sql, yard, exact_g1 = OPS[name]
    q = _q("SELECT SUM(%s), MIN(%s), MAX(%s), AVG(%s), COUNT(*) FROM t%s GROUP BY %s" % (sql, sql, sql, sql, where, group))
    mask = allc["f"] < 100 if where else np.ones(len(allc["f"]), dtype=bool)
    with np.errstate(all="ignore"):
        vals = np.asarray(yard(allc), dtype=np.float64)
    exact = group == "id" or exact_g1
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        assert p.scan_geometry()["variant"] == variant and p.group_path() == path
    want = E.group_stats([allc[group]], vals, mask)
    got = {k: v for k, v in zip(r.keys, r.values)}
    assert set(got) == set(want) and len(got) == len(r)
    if exact and group != "id":
        # every asserted sum is exactly representable: integers whose magnitudes sum below 2^53 per group, or quarters
        # below 2^51 -- or not finite, which no order of adding changes
        fin = vals[np.isfinite(vals)]
        assert np.all(fin * 4 == np.floor(fin * 4))
        bound = 2.0 ** 53 if np.all(fin == np.floor(fin)) else 2.0 ** 51
        assert all(st[4] < bound for st in want.values() if np.isfinite(st[4]))
        assert sum(np.isfinite(st[0]) for st in want.values()) >= 2
    for k, row in got.items():
        for (fn, _), v in zip(q.aggregations, row):
            _check_agg(fn, v, want[k], exact)
    assert r.stats.num_docs_scanned == int(mask.sum())


@pytest.mark.parametrize("name", list(OPS))
def test_ops_in_both_scan_instances_on_both_tables(data, name):
    t, hs, segc, allc = data
    assert 0 < int((allc["f"] < 100).sum()) < len(allc["f"]) // 5
    _run_ops(t, hs, allc, name, "g1", " WHERE f < 100", SPARSE, "lds")
    _run_ops(t, hs, allc, name, "g1", "", DENSE, "lds")
    _run_ops(t, hs, allc, name, "id", " WHERE f < 100", SPARSE, "global")
    _run_ops(t, hs, allc, name, "id", "", DENSE, "global")


def test_the_edge_values_one_by_one(data):
    """What Java documents for the ops, read back per doc (GROUP BY id) from the first docs of the first segment."""
    t, hs, segc, allc = data
    r = t.execute_groupby(hs[:1], _q("SELECT MAX(abs(d)), MAX(ceil(d)), MAX(floor(d)), MAX(sqrt(d)), MAX(mod(d, 3)), "
                                    "MAX(mod(l, -7)), MAX(timeconvert(l,'MILLISECONDS','DAYS')) FROM t WHERE id < 27 GROUP BY id"))
    got = r.as_dict()
    bits = E.canon_bits
    row = {i: got[(i,)] for i in range(27)}
    assert [bits(row[1][k]) for k in range(5)] == [bits(x) for x in (0.0, -0.0, -0.0, -0.0, -0.0)]       # d = -0.0
    assert [bits(row[3][k]) for k in range(5)] == [bits(x) for x in (0.5, -0.0, -1.0, float("nan"), -0.5)]  # d = -0.5
    assert [bits(row[2][k]) for k in range(5)] == [bits(x) for x in (0.5, 1.0, 0.0, np.sqrt(0.5), 0.5)]     # d = 0.5
    assert [bits(row[8][k]) for k in range(5)] == [bits(x) for x in (float("inf"),) * 4 + (float("nan"),)]  # d = +inf
    assert [bits(row[9][k]) for k in (0, 3, 4)] == [bits(x) for x in (float("inf"), float("nan"), float("nan"))]  # -inf
    assert all(bits(row[10][k]) == bits(float("nan")) for k in range(5))                                    # d = NaN
    assert bits(row[15][3]) == bits(np.sqrt(2.0)) == 0x3ff6a09e667f3bcd
    # truncation toward zero: -1 ms is day 0 (+0.0, not -0.0 and not -1), one day back is -1
    edges = {v: i for i, v in enumerate(L_EDGES)}
    assert bits(row[edges[-1]][6]) == bits(0.0) and bits(row[edges[-DAY + 1]][6]) == bits(0.0)
    assert row[edges[-DAY]][6] == -1.0 and row[edges[-DAY - 1]][6] == -1.0
    assert row[edges[DAY - 1]][6] == 0.0 and row[edges[DAY]][6] == 1.0 and row[edges[17428 * DAY - 1]][6] == 17427.0
    assert row[edges[2 ** 53]][6] == float(2 ** 53 // DAY) and row[edges[-2 ** 53]][6] == -float(2 ** 53 // DAY)
    # the sign of % is the dividend's: -8 % -7 is -1, 8 % -7 is 1, -7 % -7 is -0.0
    assert [bits(row[edges[v]][5]) for v in (-8, 8, -7, 7)] == [bits(x) for x in (-1.0, 1.0, -0.0, 0.0)]


# ------------------------------------------------------------------------------------------------ 3. GROUP BY
def _bucket(ts, g):
    return T.np_tdiv(ts, g) * np.int64(g)


# name -> (expression, yardstick, cardinality of the derived column in the 8229-doc segment)
BUCKETS = {
    "card1": ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:DAYS:EPOCH','1:DAYS')", lambda ts: T.np_tdiv(_bucket(ts, DAY), DAY), 1),
    "card3": ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','2:HOURS')", lambda ts: T.np_tdiv(_bucket(ts, 2 * HOUR), HOUR), 3),
    "card20": ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')", lambda ts: _bucket(ts, MIN15), 20),
    "card300": ("dateTimeConvert(ts,'1:MILLISECONDS:EPOCH','1:MINUTES:EPOCH','1:MINUTES')", lambda ts: T.np_tdiv(_bucket(ts, 60000), 60000), 300),
    "seconds": ("timeconvert(q,'DAYS','SECONDS')", None, 8),
}


@pytest.mark.parametrize("name", list(BUCKETS))
def test_derived_long_column_bytes(data, oracle, name):
    """The derived column is the LONG dictionary and forward index the segment creator writes for the yardstick's values."""
    t, hs, segc, allc = data
    expr, yard, card0 = BUCKETS[name]
    q = _q("SELECT COUNT(*) FROM t GROUP BY %s" % expr)
    gname = q.group_by[0]
    fn, rest = expr.split("(", 1)
    assert gname == fn.lower() + "(" + rest  # the lower-case function form, the string arguments as written
    t.query_c(q)
    assert t.index[("group", gname)] >= L.GROUP_EXPR_COLUMN_BASE and t.group_types[gname] == L.LONG
    bits_seen = []
    for h, cols in zip(hs, segc):
        vals = yard(cols["ts"]) if yard else cols["q"].astype(np.int64) * 86400
        want = oracle.build_column(L.LONG, vals)
        card, bits, dict_bytes, fwd_bytes = t.segment_column_bytes(h, ("group", gname))
        assert (card, bits) == (want.cardinality, want.bits_per_element)
        assert dict_bytes == want.dict_bytes and fwd_bytes == want.fwd_bytes
        bits_seen.append(bits)
        n = len(vals)
        docs = np.arange(max(0, n - 70), n)
        dvals = np.frombuffer(dict_bytes, dtype=">i8")
        assert np.array_equal(dvals[t.read_dict_ids(h, ("group", gname), docs)], vals[docs])
    assert t.segment_column_bytes(hs[0], ("group", gname))[0] == card0
    assert bits_seen[0] == max(1, int(card0 - 1).bit_length()) and bits_seen[2] == 1
    if name == "card300":
        assert bits_seen[0] == 9  # more than 8 bits


def _check_group_query(t, hs, allc, sql, keys, mask=None, projected=None, path=None):
    q = _q(sql)
    mask = np.ones(len(allc["f"]), dtype=bool) if mask is None else mask
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        if path:
            assert p.group_path() == path
    want = {}
    qv = allc["q"]
    for i in np.nonzero(mask)[0].tolist():
        w = want.setdefault(tuple(int(k[i]) for k in keys), [0, 0.0])
        w[0] += 1
        w[1] += float(qv[i])
    assert r.as_dict() == want
    assert all(type(x) is int for k in r.keys for x in k)
    assert r.stats.num_docs_scanned == int(mask.sum())
    if projected is not None:
        assert r.stats.num_entries_scanned_post_filter == int(mask.sum()) * projected
    return r, q


def test_group_by_a_time_bucket(data):
    t, hs, segc, allc = data
    b15 = "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')"
    keys = _bucket(allc["ts"], MIN15)
    # the operand ts and q are projected; the derived column is not
    r, q = _check_group_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t GROUP BY " + b15, [keys], projected=2, path="lds")
    assert len(r) == 20
    r, q = _check_group_query(t, hs, allc, "SELECT country, %s, COUNT(*), SUM(q) FROM t GROUP BY country, %s" % (b15, b15),
                              [allc["country"], keys], projected=3, path="lds")
    assert len(r) == 100
    m = allc["f"] < 300
    _check_group_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t WHERE f < 300 GROUP BY country, " + b15,
                       [allc["country"], keys], mask=m, projected=3)
    # 300 one-minute buckets beside id: past the LDS table
    minute = T.np_tdiv(_bucket(allc["ts"], 60000), 60000)
    _check_group_query(t, hs, allc, "SELECT COUNT(*), SUM(q) FROM t GROUP BY id, "
                       "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MINUTES:EPOCH','1:MINUTES')", [allc["id"], minute],
                       projected=3)
    # timeconvert of a negative column: the buckets truncate toward zero, so days -0 and +0 are one group
    days = T.np_tdiv(allc["l"], DAY)
    r, _ = _check_group_query(t, hs[1:], {k: v[DOCS[0]:] for k, v in allc.items()},
                              "SELECT COUNT(*), SUM(q) FROM t GROUP BY timeconvert(l,'MILLISECONDS','DAYS')", [days[DOCS[0]:]],
                              projected=2)
    assert r.as_dict()[(0,)][0] >= 13  # -1, 0, 1, .. DAY - 1, -DAY + 1: one bucket


def test_order_by_the_bucket_and_the_datatable_name(data):
    t, hs, segc, allc = data
    b2h = "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','2:HOURS')"
    q = _q("SELECT %s, COUNT(*) FROM t GROUP BY %s ORDER BY %s DESC LIMIT 2" % (b2h, b2h, b2h))
    q.min_server_group_trim_size = 1
    r = t.execute_groupby(hs, q)
    top = r.trim_sql()
    hours = T.np_tdiv(_bucket(allc["ts"], 2 * HOUR), HOUR)
    order = sorted(set(hours.tolist()), reverse=True)
    assert len(order) == 3 and [k[0] for k in top.keys[:2]] == order[:2]
    assert [v[0] for v in top.values[:2]] == [int((hours == k).sum()) for k in order[:2]]
    assert b2h.encode() in r.datatable()
    assert set(r.string_keys()) == {str(k) for k in order}


# ------------------------------------------------------------------------------------------------ 4. WHERE
def _model_tree(f, masks_of, masks):
    """test_expr_filter_gpu.model_tree for this file's leaves: an expression leaf is never folded, a plain leaf that
    matches no doc or every doc of the segment is an Empty / MatchAll operator."""
    if f.type == "PREDICATE":
        m, expr = masks_of(f.predicate)
        if not expr and (not m.any() or m.all()):
            return ("all",) if m.all() else ("empty",)
        masks.append(m)
        return ("expr" if expr else "scan", len(masks) - 1)
    kids = [_model_tree(k, masks_of, masks) for k in f.children]
    stop, skip = ("empty", "all") if f.type == "AND" else ("all", "empty")
    if any(k[0] == stop for k in kids):
        return (stop,)
    kids = [k for k in kids if k[0] != skip]
    if not kids:
        return (skip,)
    return kids[0] if len(kids) == 1 else ("and" if f.type == "AND" else "or", kids)


def _renumber(tree, renum):
    if tree[0] in ("and", "or"):
        return (tree[0], [_renumber(k, renum) for k in tree[1]])
    return (tree[0], renum[tree[1]])


def _filter_mask(f, masks_of):
    if f.type == "PREDICATE":
        return masks_of(f.predicate)[0]
    kids = [_filter_mask(k, masks_of) for k in f.children]
    return np.logical_and.reduce(kids) if f.type == "AND" else np.logical_or.reduce(kids)


def _entries(q, seg_cols, leaf_mask):
    """numEntriesScannedInFilter of the reference's iterators (test_expr_filter_cpu's port: an expression leaf evaluates
    blocks of 10000 docs), summed over the segments."""
    total = 0
    for cols in seg_cols:
        def masks_of(p, cols=cols):
            if p.column in q.expressions:
                return leaf_mask(cols), True
            assert p.column == "f" and p.type == "RANGE"
            return cols["f"] < int(p.values[1]), False
        masks = []
        tree = _model_tree(q.filter, masks_of, masks)
        if tree[0] not in ("empty", "all"):
            used = sorted({l[1] for l in M.leaves_of(tree)})
            renum = {old: new for new, old in enumerate(used)}
            total += M.model_entries(_renumber(tree, renum), [masks[i] for i in used])
    return total


def _days(c):
    return T.np_tdiv(c["l"], DAY)


TC = "timeconvert(l,'MILLISECONDS','DAYS')"
# name -> (predicate, the leaf's doc set over typed columns)
LEAVES = {
    "eq": (TC + " = 0", lambda c: _days(c) == 0),
    "eq_negative": (TC + " = -1", lambda c: _days(c) == -1),
    "in": (TC + " IN (1, 17427, -104249991)", lambda c: np.isin(_days(c), [1, 17427, -104249991])),
    "between": (TC + " BETWEEN -1 AND 17427", lambda c: (_days(c) >= -1) & (_days(c) <= 17427)),
    "not_in": (TC + " NOT IN (0, 1)", lambda c: ~np.isin(_days(c), [0, 1])),
    "div": ("DIV(%s,1) = 17428" % TC, lambda c: _f(_days(c)) / 1.0 == 17428.0),
    "div_in": ("DIV(%s,1) IN (0, 1)" % TC, lambda c: np.isin(_f(_days(c)) / 1.0, [0.0, 1.0])),
    "bucket": ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','2:HOURS') = %d" % (DAY0 // HOUR + 2),
               lambda c: T.np_tdiv(_bucket(c["ts"], 2 * HOUR), HOUR) == DAY0 // HOUR + 2),
    "floor": ("floor(d) = 2", lambda c: np.floor(c["d"]) == 2.0),
    "mod": ("mod(l, 2) = 0", lambda c: np.fmod(_f(c["l"]), 2.0) == 0.0),  # (a DOUBLE leaf: -0.0 == 0.0)
}


@pytest.mark.parametrize("name", list(LEAVES))
def test_where_leaves(data, name):
    t, hs, segc, allc = data
    where, leaf = LEAVES[name]
    with np.errstate(all="ignore"):
        for cond, combine in ((where, lambda m, f: m), ("%s AND f < 300" % where, lambda m, f: m & f),
                              ("f < 300 OR %s" % where, lambda m, f: m | f)):
            sql = "SELECT COUNT(*), SUM(q) FROM t WHERE %s GROUP BY g1" % cond
            mask = combine(leaf(allc), allc["f"] < 300)
            assert int(mask.sum()) < len(mask), cond
            r, q = _check_group_query(t, hs, allc, sql, [allc["g1"]], mask=mask, path="lds")
            assert r.stats.num_entries_scanned_in_filter == _entries(q, segc, leaf), cond
            if cond == where:
                assert int(mask.sum()) > 0
                assert r.stats.num_entries_scanned_in_filter == sum(DOCS)  # a lone leaf evaluates every doc: one block each
                for h, cols in zip(hs, segc):  # the doc set itself
                    n = len(cols["f"])
                    got = np.unpackbits(t.filter_bitmap(h, q, n).view(np.uint8), bitorder="little")[:n]
                    assert np.array_equal(got.astype(bool), leaf(cols)), cond


def test_a_long_leaf_declines_a_decimal_literal(data):
    t, hs, segc, allc = data
    for bad in (TC + " = 1.5", TC + " IN (1, 9223372036854775808)"):
        with pytest.raises(ValueError) as e:
            t.plan(hs, "SELECT COUNT(*) FROM t WHERE %s GROUP BY g1" % bad)
        assert "LONG literal" in str(e.value)
    # a CASE over INT branches is LONG-typed only once the column types are known: the table checks it
    q = _q("SELECT COUNT(*) FROM t WHERE CASE WHEN q > 4 THEN l ELSE 0 END = 1.5 GROUP BY g1")
    with pytest.raises(ValueError) as e:
        t.plan(hs, q)
    assert "LONG literal" in str(e.value)


# ------------------------------------------------------------------------------------------------ 5. declines
def test_registration_checks(data):
    t, hs, segc, allc = data
    C, Lt = L.EXPR_COLUMN, L.EXPR_LITERAL
    l, d = t.index["l"], t.index["d"]
    bad = [([(C, l, 0), (C, l, 0), (L.EXPR_LDIV, 0, 0)], "LITERAL right before it"),
           ([(C, l, 0), (Lt, 0, 0.0), (L.EXPR_LDIV, 0, 0)], "positive integer"),
           ([(C, l, 0), (Lt, 0, 2.0 ** 53 + 2), (L.EXPR_LDIV, 0, 0)], "2^53"),
           ([(C, l, 0), (Lt, 0, 2.5), (L.EXPR_MULT, 0, 0), (Lt, 0, 7.0), (L.EXPR_LDIV, 0, 0)], "integral"),
           ([(C, d, 0), (Lt, 0, 7.0), (L.EXPR_LDIV, 0, 0)], "integral"),  # a DOUBLE column: the table knows its type
           ([(C, d, 0), (Lt, 0, 3.0), (L.EXPR_MULT, 0, 0), (Lt, 0, 7.0), (L.EXPR_LDIV, 0, 0)], "integral"),
           ([(C, l, 0), (C, l, 0), (L.EXPR_GT, 0, 0), (L.EXPR_FLOOR, 0, 0)], "not booleans"),
           ([(C, l, 0), (C, l, 0), (15, 0, 0)], "unknown op"), ([(C, l, 0), (C, l, 0), (22, 0, 0)], "unknown op")]
    for ops, word in bad:
        for add in (t.add_expression, lambda o: t.add_group_expression(o, "LONG")):
            with pytest.raises(L.PinotGpuError) as e:
                add(ops)
            assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and word in str(e.value), (ops, str(e.value))
    col = t.add_expression([(C, l, 0), (Lt, 0, 7.0), (L.EXPR_LDIV, 0, 0), (L.EXPR_ABS, 0, 0), (C, d, 0), (L.EXPR_MOD, 0, 0)])
    assert t.expression(col)[1] == "mod(abs(ldiv(l,7)),d)"  # the name built from the program


def test_plan_time_range_check(oracle, gpu_lib):
    """A LONG column within +-2^53 whose values times the input factor pass 2^53: declined per plan, as an aggregation,
    as a leaf and as a GROUP BY, with the table and the other plans working afterwards."""
    schema = [("g", "INT"), ("big", "LONG"), ("small", "LONG")]
    n = 100
    cols = {"g": np.arange(n) % 3, "big": np.arange(n, dtype=np.int64) * (1 << 24) - (1 << 30),
            "small": np.arange(n, dtype=np.int64) * 1000}
    conv = "datetimeconvert(%s,'1:DAYS:EPOCH','1:HOURS:EPOCH','1:HOURS')"
    assert int(np.abs(cols["big"]).max()) * DAY > 2 ** 53 > int(np.abs(cols["small"]).max()) * DAY
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        for sql, word in (("SELECT SUM(%s) FROM t GROUP BY g" % (conv % "big"), "expression"),
                          ("SELECT MAX(timeconvert(big,'DAYS','MILLISECONDS')) FROM t GROUP BY g", "expression"),
                          ("SELECT COUNT(*) FROM t WHERE %s = 5 GROUP BY g" % (conv % "big"), "expression"),
                          ("SELECT COUNT(*) FROM t GROUP BY %s" % (conv % "big"), "GROUP BY expression")):
            with pytest.raises(L.UnsupportedQueryError) as e:
                t.plan([h], _q(sql))
            assert e.value.code == L.PGPU_ERR_UNSUPPORTED and word in str(e.value) and "2^53" in str(e.value), str(e.value)
            assert ("GROUP BY expression" in str(e.value)) == (word == "GROUP BY expression")
            # the table and the other plans still work
            r = t.execute_groupby([h], _q("SELECT COUNT(*), MAX(%s) FROM t GROUP BY g" % (conv % "small")))
            assert r.as_dict() == {(k,): [int((cols["g"] == k).sum()), float(cols["small"][cols["g"] == k].max() * 24)]
                                   for k in range(3)}
        r = t.execute_groupby([h], _q("SELECT COUNT(*) FROM t GROUP BY %s" % (conv % "small")))
        assert r.as_dict() == {(int(v) * 24,): [1] for v in cols["small"]}
        # the division alone keeps big within range: it runs
        r = t.execute_groupby([h], _q("SELECT COUNT(*) FROM t GROUP BY timeconvert(big,'SECONDS','DAYS')"))
        days = T.np_tdiv(cols["big"], 86400)
        assert r.as_dict() == {(int(k),): [int((days == k).sum())] for k in set(days.tolist())}


# ------------------------------------------------------------------------------------------------ 6. the plan cache
def test_plan_cache_and_two_granularities(data):
    t, hs, segc, allc = data
    sql = "SELECT COUNT(*), SUM(q), MAX(%s) FROM t WHERE f < 500 GROUP BY datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','%s')"
    a = t.execute_groupby(hs, _q(sql % (TC, "1:HOURS")))
    ia = t.index[("group", _q(sql % (TC, "1:HOURS")).group_by[0])]
    b = t.execute_groupby(hs, _q(sql % (TC, "1:HOURS")))  # the same bytes: a plan-cache hit
    assert t.index[("group", _q(sql % (TC, "1:HOURS")).group_by[0])] == ia
    c = t.execute_groupby(hs, _q(sql % (TC, "2:HOURS")))
    ic = t.index[("group", _q(sql % (TC, "2:HOURS")).group_by[0])]
    assert ia != ic and a.as_dict() == b.as_dict() and len(a) == 5 and len(c) == 3
    m = allc["f"] < 500
    for r, g in ((a, HOUR), (c, 2 * HOUR)):
        hours = T.np_tdiv(_bucket(allc["ts"], g), HOUR)
        days = _f(_days(allc))
        assert r.as_dict() == {(int(k),): [int((m & (hours == k)).sum()), float(allc["q"][m & (hours == k)].sum()),
                                           float(days[m & (hours == k)].max())] for k in set(hours[m].tolist())}
