"""PERCENTILE on the GPU group-by path: the reference's recorded answers (InterSegmentAggregationSingleValueQueriesTest.
testPercentile50 / 90 / 95 / 99, tests/golden/kat_inter_percentile.json) and a numpy sort per group indexed by the Java
formula (percentile_common.py) -- the oracle has no PERCENTILE.  The result is a column value, not a sum: compared with
==.  Each test asserts through Plan.group_path / Plan.scan_geometry()["variant"] (10 sparse, 11 dense: the histogram
instances of k_direct.hip) the path it means to cover."""
import numpy as np
import pytest

import distinct_common as D
import kat_common as K
import percentile_common as P
import startree_common as SC
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import QueryContext, parse_query
from pinot_amd.startree import StarTree

pytestmark = pytest.mark.gpu
SPARSE, DENSE = 10, 11
STEP_CELLS = 256  # cells one wave step of percentile_select_kernel covers: 64 lanes x one 16-byte load of 4 cells
BATCH_STEPS = 8   # steps whose loads the kernel issues together

# test_distinct_count_gpu.py's shape: two segments whose local dictionaries of v (and s) overlap only partly -- segment 0
# holds values 0..39, segment 1 30..129, so a local dictId is not the global one.  8192 + 37 docs: one whole tile and a
# tail; 100 docs: a lane tail.  m is negative in half its docs; vl lies beyond 2^53, where (double)value rounds.
SCHEMA = [("g1", "INT"), ("g2", "INT"), ("v", "INT"), ("s", "STRING"), ("m", "INT"), ("md", "DOUBLE"), ("f", "INT"),
          ("vl", "LONG")]
DOCS = (8192 + 37, 100)
RANGES = ((0, 40), (30, 130))
PCTS = (0, 50, 90, 99.9, 100)


def _columns(rng, n, lo, hi):
    v = rng.integers(lo, hi, n)
    v[:hi - lo] = np.arange(lo, hi)[:n]  # (every value of the range where the segment has the docs)
    return {"g1": rng.integers(0, 7, n), "g2": rng.integers(10, 15, n), "v": v,
            "s": ["s%03d" % x for x in rng.integers(lo, hi, n)], "m": rng.integers(-500, 500, n),
            "md": rng.uniform(-10, 10, n), "f": rng.integers(0, 1000, n),
            "vl": (1 << 60) + rng.integers(0, 4000, n).astype(np.int64) * 3 + 1}


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(5)
    cols = [_columns(rng, n, lo, hi) for n, (lo, hi) in zip(DOCS, RANGES)]
    segs = [oracle.make_segment(SCHEMA, c) for c in cols]
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(s) for s in segs]
    allc = {name: (np.concatenate([c[name] for c in cols]) if typ != "STRING" else sum([c[name] for c in cols], []))
            for name, typ in SCHEMA}
    yield t, hs, segs, allc
    t.close()


def _mask(allc, f_below):
    return np.ones(len(allc["f"]), dtype=bool) if f_below is None else allc["f"] < f_below


def _where(f_below):
    return "" if f_below is None else " WHERE f < %d" % f_below


def _run(t, hs, q):
    """(as_dict, stats tuple, group path, scan instance) of q."""
    with t.plan(hs, q) as p:
        p.execute()
        r = p.finalize()
        return r.as_dict(), r.stats.as_tuple(), p.group_path(), p.scan_geometry()["variant"]


def _expected(allc, group_by, items, m):
    """{key: [value per (column, percentile) of items]} by the numpy yardstick."""
    per = [P.percentiles([allc[c] for c in group_by], allc[c], m, p) for c, p in items]
    return {k: [x[k] for x in per] for k in per[0]}


def _select(items):
    return ", ".join("PERCENTILE(%s, %s)" % (c, p) for c, p in items)


# ------------------------------------------------------------------------------------------------ the reference's KAT
@pytest.fixture(scope="module")
def sv(oracle, gpu_lib):
    t = GpuTable(K.SCHEMA)
    h = t.pin_segment(K.kat_segment(oracle, pairs=True))
    yield t, h
    t.close()


@pytest.mark.parametrize("case", P.KAT_PERCENTILE["cases"], ids=lambda c: "%s-%s" % (c["test"], c["variant"]))
def test_kat_inter_segment_percentile(sv, case):
    """InterSegmentAggregationSingleValueQueriesTest.java:245-332: values and the full statistics tuple, for every
    spelling the reference runs."""
    t, h = sv
    for sql in [case["query"]] + case.get("spellings", []):
        q = parse_query(sql)
        if case["filter"]:
            q.filter = QueryContext.filter_from_json(K.KAT["query_filter"])
        if case["group_by"]:
            q.group_by = [P.KAT_PERCENTILE["group_by_column"]]
        with t.plan([h] * 4, q) as p:
            p.execute()
            r = p.finalize()
            assert p.group_path() in ("lds", "global")
            assert p.scan_geometry()["variant"] in (SPARSE, DENSE)
        rows = r.values
        assert all(isinstance(x, float) for row in rows for x in row)
        top = [max(row[a] for row in rows) for a in range(2)]  # PQL: the top group per function
        assert ["%.5f" % x for x in top] == case["values"]
        assert top == [float(x) for x in case["values"]]
        assert tuple(r.stats.as_tuple()[:4]) == tuple(case["stats"])


# ------------------------------------------------------------------------------------------------ numpy parity
@pytest.mark.parametrize("group_by", [["g1"], ["g1", "g2"]], ids=["one_key", "two_keys"])
@pytest.mark.parametrize("f_below", [None, 150], ids=["all", "f15"])
@pytest.mark.parametrize("col", ["v", "md", "vl", "m"], ids=["int", "double", "long_past_2p53", "negative"])
def test_parity(data, group_by, f_below, col):
    t, hs, segs, allc = data
    items = [(col, p) for p in PCTS]
    q = parse_query("SELECT %s FROM t%s GROUP BY %s" % (_select(items), _where(f_below), ", ".join(group_by)))
    got, stats, path, variant = _run(t, hs, q)
    m = _mask(allc, f_below)
    assert got == _expected(allc, group_by, items, m)
    assert all(isinstance(x, float) for row in got.values() for x in row)
    assert path == "lds" and variant == (DENSE if f_below is None else SPARSE)
    # numEntriesScannedPostFilter: docs x distinct group-by and aggregation columns
    assert stats[0] == int(m.sum()) and stats[2] == int(m.sum()) * (len(group_by) + 1)
    if col == "vl":  # the data does round: (double)value is not the value
        assert any(int(x) != v for x, v in zip(allc["vl"].astype(np.float64).tolist(), allc["vl"].tolist()))
    if col == "m":
        assert min(row[0] for row in got.values()) < 0 < max(row[4] for row in got.values())


# ------------------------------------------------------------------------------------------------ selection kernel
@pytest.mark.parametrize("card", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2 * STEP_CELLS + 1,
                                  BATCH_STEPS * STEP_CELLS + 1])
def test_cardinality_edges(oracle, gpu_lib, card):
    """Global cardinalities around the 4-cell load, the 64-cell lane boundary and the 256-cell wave step (257: one
    cell past a step; 513: one past two; 2049: one past the 8 steps loaded together); the two local dictionaries
    overlap partly."""
    rng = np.random.default_rng(card)
    schema = [("g", "INT"), ("v", "INT")]
    # segment 0 (8229 docs) holds global values [0, a_hi), segment 1 (100 docs) the last <= 60, overlapping by <= 30
    a_hi, b_lo = max(1, min(card, max((2 * card) // 5, card - 30))), max((3 * card) // 10, card - 60)
    cols = []
    for n, (lo, hi) in zip(DOCS, ((0, a_hi), (b_lo, card))):
        v = rng.integers(lo, hi, n)
        v[:min(hi - lo, n)] = np.arange(lo, hi)[:n]
        cols.append({"g": rng.integers(0, 3, n), "v": v * 7 - 100})
    with GpuTable(schema) as t:
        hs = [t.pin_segment(oracle.make_segment(schema, c)) for c in cols]
        assert len(t.dictionary("v")) == card
        items = [("v", p) for p in (0, 12.5, 50, 99.99, 100)]
        got, _, path, variant = _run(t, hs, parse_query("SELECT %s FROM t GROUP BY g" % _select(items)))
        allc = {k: np.concatenate([c[k] for c in cols]) for k in ("g", "v")}
        assert got == _expected(allc, ["g"], items, np.ones(len(allc["g"]), dtype=bool))
        assert path == "lds" and variant == DENSE
        # G == 1: p100 is the row's last cell, p0 its first
        tot = t.execute_aggregation(hs, parse_query("SELECT PERCENTILE100(v), PERCENTILE0(v) FROM t"))
        assert tot.values == [float(allc["v"].max()), float(allc["v"].min())]


def test_target_cells_and_an_empty_group(oracle, gpu_lib):
    """513 global values; per group the docs are placed so that the target is the row's first cell, its last cell,
    the last cell of a wave step (global dictId 255) and the first of the next (256), and a cell whose count straddles
    the target index (1000 duplicates).  Group 5 has docs, none of which passes the filter: absent, beside present ones."""
    card = 2 * STEP_CELLS + 1
    vals = np.arange(card) * 3 + 11  # global dictId g holds value 3 g + 11
    g, v, f = [], [], []

    def add(group, gids_counts, keep=1):
        for gid, cnt in gids_counts:
            g.extend([group] * cnt)
            v.extend([int(vals[gid])] * cnt)
            f.extend([keep] * cnt)

    add(0, [(0, 6), (300, 4)])                      # p50 -> index 5: the row's first cell
    add(1, [(3, 4), (card - 1, 6)])                 # p50 -> index 5: the row's last cell
    add(2, [(STEP_CELLS - 1, 10), (STEP_CELLS, 10)])  # p45 -> index 9: dictId 255; p50 -> index 10: dictId 256
    add(3, [(5, 1), (7, 1000), (9, 1)])             # p50 -> index 501, inside the 1000 docs of dictId 7
    add(4, [(i, 1) for i in range(card)])           # every value once (the whole dictionary is in the segment)
    add(5, [(100, 50)], keep=0)                     # no doc passes the filter
    schema = [("g", "INT"), ("v", "INT"), ("f", "INT")]
    cols = {"g": np.array(g), "v": np.array(v), "f": np.array(f)}
    rng = np.random.default_rng(2)
    order = rng.permutation(len(g))
    cols = {k: c[order] for k, c in cols.items()}
    items = [("v", 45), ("v", 50)]
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        assert len(t.dictionary("v")) == card
        got, _, path, variant = _run(t, [h], parse_query("SELECT %s FROM t WHERE f = 1 GROUP BY g" % _select(items)))
    assert variant in (SPARSE, DENSE) and path == "lds"
    assert got == _expected(cols, ["g"], items, cols["f"] == 1)
    assert sorted(got) == [(0,), (1,), (2,), (3,), (4,)]  # group 5 is absent
    assert got[(0,)][1] == float(vals[0]) and got[(1,)][1] == float(vals[card - 1])
    assert got[(2,)] == [float(vals[STEP_CELLS - 1]), float(vals[STEP_CELLS])]
    assert got[(3,)][1] == float(vals[7])


def test_java_double_arithmetic(oracle, gpu_lib):
    """A group of exactly 10000 docs with distinct values: PERCENTILE(v, 0.57) is the value at sorted index 56, because
    10000 * 0.57 is 5699.99... in doubles; the exact rational floor says 57."""
    assert 10000 * 57 // 10000 == 57 and P.java_index(10000, 0.57) == 56
    rng = np.random.default_rng(9)
    schema = [("g", "INT"), ("v", "INT")]
    v0 = rng.permutation(10000) * 2 + 1
    cols = {"g": np.concatenate([np.zeros(10000, dtype=np.int64), np.ones(321, dtype=np.int64)]),
            "v": np.concatenate([v0, rng.integers(0, 20000, 321)])}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        got, stats, _, variant = _run(t, [h], parse_query("SELECT PERCENTILE(v, 0.57), COUNT(*) FROM t GROUP BY g"))
    assert variant == DENSE and got[(0,)][1] == 10000
    assert got[(0,)][0] == float(np.sort(v0)[56]) == 113.0
    assert got[(0,)][0] != float(np.sort(v0)[57])
    assert got[(1,)][0] == P.percentiles([cols["g"]], cols["v"], cols["g"] == 1, 0.57)[(1,)]


# ------------------------------------------------------------------------------------------------ aggregation paths
@pytest.mark.parametrize("f_below,dense_sel,variant", [(10, 0.25, SPARSE), (150, 0.25, SPARSE), (150, 0.1, DENSE),
                                                       (None, 0.25, DENSE)],
                         ids=["queue_1pct", "batch_15pct", "dense_instance_15pct", "dense_all"])
def test_each_aggregation_path(data, f_below, dense_sel, variant):
    """~1 %: the wave queue (flush_wave_queue); ~15 %: lanes with more than 2 matches (aggregate_batch), in the sparse
    and -- dense_selectivity lowered -- the dense instance, whose wave-tiles past 256 matches decode whole groups;
    no filter: aggregate_group on every full tile."""
    t, hs, segs, allc = data
    items = [("v", 50), ("v", 95)]
    q = parse_query("SELECT COUNT(*), %s FROM t%s GROUP BY g1, g2" % (_select(items), _where(f_below)))
    m = _mask(allc, f_below)
    if f_below == 150:  # some lane's 32-doc group holds more than 2 matches
        assert np.add.reduceat(m[:8192].astype(int), np.arange(0, 8192, 32)).max() > 2
    t.set_config(dense_selectivity=dense_sel)
    try:
        got, _, path, v = _run(t, hs, q)
    finally:
        t.reset_config()
    exp = _expected(allc, ["g1", "g2"], items, m)
    counts = D.distinct_counts([allc["g1"], allc["g2"]], [np.arange(len(m))], m)  # (COUNT(*): the docs are distinct)
    assert got == {k: counts[k] + exp[k] for k in exp}
    assert path == "lds" and v == variant


def test_lds_and_global_tables_agree(data):
    """lds_table_kb at its smallest value (1 KB): the 35-key table no longer fits, the plan takes global atomics."""
    t, hs, segs, allc = data
    items = [("v", 50), ("md", 90)]
    for f_below in (None, 150):
        q = parse_query("SELECT COUNT(*), %s, SUM(m) FROM t%s GROUP BY g1, g2" % (_select(items), _where(f_below)))
        lds, _, p0, v0 = _run(t, hs, q)
        t.set_config(lds_table_kb=1)
        try:
            glb, _, p1, v1 = _run(t, hs, q)
        finally:
            t.reset_config()
        assert (p0, p1) == ("lds", "global") and v0 == v1 == (DENSE if f_below is None else SPARSE)
        assert lds == glb
        exp = _expected(allc, ["g1", "g2"], items, _mask(allc, f_below))
        assert {k: v[1:3] for k, v in glb.items()} == exp


def test_shared_histogram(data):
    """Three percentiles of one column and its MAX in one query: one histogram, three rows; p100 is MAX, p0 is MIN."""
    t, hs, segs, allc = data
    q = parse_query("SELECT PERCENTILE50(v), PERCENTILE95(v), PERCENTILE(v, 99.9), MAX(v), PERCENTILE100(v), "
                    "PERCENTILE0(v), MIN(v) FROM t WHERE f < 500 GROUP BY g1, g2")
    got, stats, path, variant = _run(t, hs, q)
    m = allc["f"] < 500
    exp = _expected(allc, ["g1", "g2"], [("v", 50), ("v", 95), ("v", 99.9), ("v", 100), ("v", 0)], m)
    assert set(got) == set(exp) and variant in (SPARSE, DENSE)
    for k, row in got.items():
        assert row[:3] == exp[k][:3]
        assert row[4] == row[3] == exp[k][3] and row[5] == row[6] == exp[k][4]
    assert stats[2] == int(m.sum()) * 3  # g1, g2, v
    assert len({tuple(r[:3]) for r in got.values()}) > 1 and any(r[0] != r[1] for r in got.values())


def test_beside_other_aggregations(oracle, data):
    """PERCENTILE beside SUM, AVG, MIN and two DISTINCTCOUNTs (one over the percentile's column: they share its
    histogram): the others equal the oracle's for the query without the side functions; groups without a match are
    absent."""
    t, hs, segs, allc = data
    where = " WHERE f < 150 AND g1 <> 3"
    q = parse_query("SELECT SUM(m), PERCENTILE90(v), AVG(md), DISTINCTCOUNT(s), DISTINCTCOUNT(v), MIN(v) FROM t%s "
                    "GROUP BY g1, g2" % where)
    q0 = parse_query("SELECT SUM(m), AVG(md), MIN(v) FROM t%s GROUP BY g1, g2" % where)
    got, stats, path, variant = _run(t, hs, q)
    o = oracle.run_groupby(SCHEMA, segs, q0)
    m = (allc["f"] < 150) & (allc["g1"] != 3)
    dc = D.distinct_counts([allc["g1"], allc["g2"]], [allc["s"], allc["v"]], m)
    pc = P.percentiles([allc["g1"], allc["g2"]], allc["v"], m, 90)
    assert set(got) == set(dc) == set(pc) == set(o.groups)
    assert not any(k[0] == 3 for k in got)
    for k, row in got.items():
        assert row[1] == pc[k] and isinstance(row[1], float)
        assert [row[3], row[4]] == dc[k] and isinstance(row[3], int)
        assert row[0] == o.groups[k][0] and row[5] == o.groups[k][2]
        assert row[2].count == o.groups[k][1].count and row[2].sum == pytest.approx(o.groups[k][1].sum, rel=1e-9)
    assert stats[0] == o.stats[0] == int(m.sum()) and stats[1] == o.stats[1]
    assert variant == SPARSE and path == "lds"


def test_aggregation_only(data):
    """G == 1: with a filter, without one (scanned: docs x columns entries post filter, not 0), and with no doc matched
    (the function's default, -inf)."""
    t, hs, segs, allc = data
    for f_below in (None, 150, 10):
        q = parse_query("SELECT PERCENTILE50(v), PERCENTILE(md, 99.9), MAX(v) FROM t%s" % _where(f_below))
        with t.plan(hs, q) as p:
            p.execute()
            r = p.finalize()
            assert p.group_path() == "lds" and p.scan_geometry()["variant"] == (DENSE if f_below is None else SPARSE)
        m = _mask(allc, f_below)
        assert r.values[0][:2] == _expected(allc, [], [("v", 50), ("md", 99.9)], m)[()]
        assert r.stats.as_tuple()[0] == int(m.sum()) and r.stats.as_tuple()[2] == int(m.sum()) * 2
    n = len(allc["v"])
    only = t.execute_aggregation(hs, parse_query("SELECT PERCENTILE95(v) FROM t"))
    assert only.values == _expected(allc, [], [("v", 95)], _mask(allc, None))[()]
    assert only.stats.as_tuple()[2] == n  # not answered from the dictionary
    none = t.execute_aggregation(hs, parse_query("SELECT PERCENTILE95(v), COUNT(*) FROM t WHERE f > 5000"))
    assert none.values == [float("-inf"), 0] and none.stats.num_docs_scanned == 0


# ------------------------------------------------------------------------------------------------ execution hygiene
def test_reexecution_and_plan_cache(data):
    """Execute twice, then finalize: the COUNT row starts over with every execution, so a histogram that did not would
    hold two docs per doc and the target index would select the value at half the percentile.  Then three queries in
    turn through the table's one arena: the second sees other docs than the first left in the histogram."""
    t, hs, segs, allc = data
    sql = "SELECT PERCENTILE50(v), PERCENTILE90(md), COUNT(*) FROM t WHERE f %s 400 GROUP BY g1"
    q, q2 = parse_query(sql % "<"), parse_query(sql % ">=")
    items = [("v", 50), ("md", 90)]
    exp, exp2 = _expected(allc, ["g1"], items, allc["f"] < 400), _expected(allc, ["g1"], items, allc["f"] >= 400)
    half = _expected(allc, ["g1"], [("v", 25), ("md", 45)], allc["f"] < 400)
    assert all(exp[k] != half[k] for k in exp)  # a doubled histogram would show
    with t.plan(hs, q) as p:
        p.execute()
        p.execute()
        assert {k: v[:2] for k, v in p.finalize().as_dict().items()} == exp
    a = t.execute_groupby(hs, q).as_dict()
    b = t.execute_groupby(hs, q2).as_dict()
    c = t.execute_groupby(hs, q).as_dict()  # a plan-cache hit
    assert {k: v[:2] for k, v in a.items()} == exp and a == c
    assert {k: v[:2] for k, v in b.items()} == exp2 and exp != exp2


def test_two_plans_in_flight_on_two_streams(data):
    import torch
    t, hs, segs, allc = data
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    q1 = parse_query("SELECT PERCENTILE50(v) FROM t WHERE f < 150 GROUP BY g1, g2")
    q2 = parse_query("SELECT PERCENTILE50(v) FROM t WHERE f >= 150 GROUP BY g1, g2")
    p1 = t.plan_execute(hs, q1, stream=s1.cuda_stream)
    p2 = t.plan_execute(hs, q2, stream=s2.cuda_stream)
    try:
        r2 = p2.finalize(s2.cuda_stream).as_dict()
        r1 = p1.finalize(s1.cuda_stream).as_dict()
    finally:
        p1.close()
        p2.close()
    assert r1 == _expected(allc, ["g1", "g2"], [("v", 50)], allc["f"] < 150)
    assert r2 == _expected(allc, ["g1", "g2"], [("v", 50)], allc["f"] >= 150)
    assert r1 != r2


def test_segment_with_a_star_tree_is_scanned(oracle, gpu_lib):
    rng = np.random.default_rng(11)
    cols = SC.c4_columns(rng, 6000, cards=(12, 6, 5, 4))
    seg = oracle.make_segment(SC.C4_SCHEMA, cols)
    star = StarTree.build(SC.C4_SCHEMA, seg, SC.C4_SPLIT, SC.C4_PAIRS, max_leaf_records=100)
    with GpuTable(SC.C4_SCHEMA) as t:
        h = t.pin_segment(seg)
        t.attach_startree(h, star)
        with t.plan([h], parse_query("SELECT COUNT(*) FROM t GROUP BY d4")) as p:
            p.execute()
            p.finalize()
            assert p.star_work()[0] == 1  # the control: the same shape without the function takes the star-tree
        with t.plan([h], parse_query("SELECT COUNT(*), PERCENTILE50(m) FROM t GROUP BY d4")) as p:
            p.execute()
            r = p.finalize()
            assert p.star_work()[0] == 0 and p.scan_geometry()["variant"] == DENSE
        exp = P.percentiles([cols["d4"]], cols["m"], np.ones(6000, dtype=bool), 50)
        assert {k: v[1] for k, v in r.as_dict().items()} == exp
        assert r.stats.num_docs_scanned == 6000


def test_order_by_percentile_desc_limit(data):
    t, hs, segs, allc = data
    q = parse_query("SELECT g1, g2, PERCENTILE95(v) FROM t WHERE f < 30 GROUP BY g1, g2 "
                    "ORDER BY PERCENTILE(v, 95) DESC LIMIT 3")
    q.min_server_group_trim_size = 1  # the server keeps max(limit * 5, 1) = 15 groups
    res = t.execute_groupby(hs, q)
    top = res.trim_sql()
    exp = P.percentiles([allc["g1"], allc["g2"]], allc["v"], allc["f"] < 30, 95)
    # descending value; ties by the composite key (the last group-by column the most significant)
    order = sorted(exp.items(), key=lambda kv: (-kv[1], kv[0][1], kv[0][0]))
    assert len(top) == 15
    assert top.keys[:3] == [k for k, _ in order[:3]]
    assert [v[0] for v in top.values[:3]] == [v for _, v in order[:3]]
    assert len(set(exp.values())) < len(exp)  # the data has ties
    # the PQL trim takes the largest values first, as for MAX
    pql = res.trim_pql(3, final=True)[0]
    assert [v for _, v in pql] == [v for _, v in order[:3]]


# ------------------------------------------------------------------------------------------------ declined shapes
def _declined(fn):
    with pytest.raises(L.UnsupportedQueryError) as e:
        fn()
    assert "PERCENTILE" in str(e.value), str(e.value)


def test_declined_histogram_cap(oracle, gpu_lib):
    """1024 x 1024 keys: 260 cells of 4 bytes per key are 1.09e9 bytes, above the 1 GiB cap (the smallest stride past
    it: strides are multiples of 4 cells); 256 cells are exactly 1 GiB, which plans."""
    schema = [("a", "INT"), ("b", "INT"), ("v", "INT"), ("w", "INT")]
    n = 16384
    cols = {"a": np.arange(n) % 1024, "b": (np.arange(n) // 16) % 1024, "v": np.arange(n) % 257, "w": np.arange(n) % 256}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        _declined(lambda: t.plan([h], parse_query("SELECT PERCENTILE50(v) FROM t GROUP BY a, b", num_groups_limit=10 ** 9)))
        with t.plan([h], parse_query("SELECT PERCENTILE50(w) FROM t GROUP BY a, b", num_groups_limit=10 ** 9)) as p:
            assert p.group_path() == "global" and p.layout()[1] == 1024 * 1024


def test_declined_hash_key_space(oracle, gpu_lib):
    """9000 x 9000 keys: past every dense table."""
    schema = [("h1", "INT"), ("h2", "INT"), ("v", "INT")]
    n = 9000
    cols = {"h1": np.arange(n), "h2": np.arange(n)[::-1].copy(), "v": np.arange(n) % 50}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        with t.plan([h], parse_query("SELECT COUNT(*) FROM t GROUP BY h1, h2", num_groups_limit=10 ** 9)) as p:
            assert p.group_path() in ("hash", "hash_partitioned")
        _declined(lambda: t.plan([h], parse_query("SELECT PERCENTILE50(v) FROM t GROUP BY h1, h2",
                                                  num_groups_limit=10 ** 9)))


def test_declined_array_map_stages(sv):
    t, h = sv
    case = K.KAT["inner_segment_group_by"][3]  # 9 group-by columns: the cardinality product overflows a long
    q = QueryContext(case["group_by"], [("PERCENTILE50", "column1")], None, num_groups_limit=10 ** 9)
    _declined(lambda: t.plan([h], q))


def test_declined_num_groups_limit(sv):
    t, h = sv
    q = QueryContext(["column1"], [("COUNT", "*"), ("PERCENTILE50", "column3")], None, num_groups_limit=1000)
    _declined(lambda: t.plan([h], q))
    _declined(lambda: t.execute_groupby([h], q))


def test_declined_string_raw_column_and_exact_fp_sum(oracle, data):
    from pinot_amd.segment import SegmentBuffers, build_raw_column
    t, hs, segs, allc = data
    _declined(lambda: t.plan(hs, parse_query("SELECT PERCENTILE50(s) FROM t GROUP BY g1")))
    q = parse_query("SELECT SUM(md), PERCENTILE50(v) FROM t GROUP BY g1", exact_fp_sum=True)
    _declined(lambda: t.plan(hs, q))
    schema = [("g", "INT"), ("r", "LONG")]
    vals = np.arange(64, dtype=np.int64) * 3
    base = oracle.make_segment([("g", "INT")], {"g": np.arange(64) % 4})
    cols = {**base.columns, "r": build_raw_column("LONG", vals.tolist(), 2)}
    with GpuTable(schema) as t2:
        h = t2.pin_segment(SegmentBuffers(64, cols))
        assert t2.execute_groupby([h], parse_query("SELECT SUM(r) FROM t GROUP BY g")).as_dict()[(0,)] == [int(vals[::4].sum())]
        _declined(lambda: t2.plan([h], parse_query("SELECT PERCENTILE50(r) FROM t GROUP BY g")))


def test_invalid_percentile_code_at_the_abi(data):
    """A code above 1000000 in pgpu_agg.fn (the Python layer never sends one): PGPU_ERR_INVALID_ARGUMENT."""
    t, hs, segs, allc = data
    q = parse_query("SELECT PERCENTILE50(v) FROM t GROUP BY g1")
    to_c = q.to_c

    def bad(index):
        c, keep = to_c(index)
        c.aggs[0].fn = L.AGG_PERCENTILE | (1000001 << 8)
        return c, keep

    q.to_c = bad
    with pytest.raises(L.PinotGpuError) as e:
        t.plan(hs, q)
    assert not isinstance(e.value, L.UnsupportedQueryError) and "PERCENTILE" in str(e.value)


def test_declined_external_merges(data):
    """finalize_range, an external d_table (execute, finalize, create_execute), exchange_counts, datatable(), and
    combine_mode / combine on a one-rank host communicator."""
    import torch
    from pinot_amd.combine import Communicator, combine_mode, combine_plan
    t, hs, segs, allc = data
    q = parse_query("SELECT COUNT(*), PERCENTILE50(v) FROM t GROUP BY g1, g2")
    d = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    _declined(lambda: t.plan_execute(hs, q, d_table=d.data_ptr()))
    comm = Communicator(L.COMM_HOST, Communicator.unique_id(L.COMM_HOST), 1, 0, 0)
    try:
        with t.plan(hs, q) as p:
            ns, nk, kinds = p.layout()
            assert (ns, nk, kinds) == (2, 35, [L.SLOT_COUNT, L.SLOT_SUM_F64])  # a float64 row to everything downstream
            _declined(lambda: p.execute(None, d.data_ptr()))
            p.execute()
            _declined(lambda: p.finalize(None, d.data_ptr()))
            _declined(lambda: p.finalize_range(None, d.data_ptr(), 0, nk))
            _declined(lambda: p.exchange_counts(None, 2))
            _declined(lambda: combine_mode(p, comm, 1 << 62))
            _declined(lambda: combine_plan(p, comm, None, 0))
            r = p.finalize()
            _declined(r.datatable)
            assert {k: v[1:] for k, v in r.as_dict().items()} == \
                _expected(allc, ["g1", "g2"], [("v", 50)], _mask(allc, None))
    finally:
        comm.close()
