"""DISTINCTCOUNT on the GPU group-by path: the reference's recorded answers (InterSegmentAggregationSingleValueQueriesTest.
testDistinctCount, tests/golden/kat_inter_distinct.json) and a brute-force numpy set count (distinct_common.py) -- the
oracle has no DISTINCTCOUNT.  Counts are integers and compared exactly.  Each test asserts through Plan.group_path /
Plan.scan_geometry()["variant"] (8 sparse, 9 dense: the DC instances of k_direct.hip) the path it means to cover."""
import numpy as np
import pytest

import distinct_common as D
import kat_common as K
import startree_common as SC
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import QueryContext, parse_query
from pinot_amd.startree import StarTree

pytestmark = pytest.mark.gpu
SPARSE, DENSE = 8, 9

# Two segments whose local dictionaries of v (and s) overlap only partly: segment 0 holds values 0..39, segment 1
# 30..129, so a local dictId is not the global one.  8192 + 37 docs: one whole tile and a tail; 100 docs: a lane tail.
SCHEMA = [("g1", "INT"), ("g2", "INT"), ("v", "INT"), ("s", "STRING"), ("m", "INT"), ("md", "DOUBLE"), ("f", "INT")]
DOCS = (8192 + 37, 100)
RANGES = ((0, 40), (30, 130))


def _columns(rng, n, lo, hi):
    v = rng.integers(lo, hi, n)
    v[:hi - lo] = np.arange(lo, hi)[:n]  # (every value of the range where the segment has the docs)
    return {"g1": rng.integers(0, 7, n), "g2": rng.integers(10, 15, n), "v": v,
            "s": ["s%03d" % x for x in rng.integers(lo, hi, n)], "m": rng.integers(-500, 500, n),
            "md": rng.uniform(-10, 10, n), "f": rng.integers(0, 1000, n)}


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


# ------------------------------------------------------------------------------------------------ the reference's KAT
@pytest.fixture(scope="module")
def sv(oracle, gpu_lib):
    t = GpuTable(K.SCHEMA)
    h = t.pin_segment(K.kat_segment(oracle, pairs=True))
    yield t, h
    t.close()


@pytest.mark.parametrize("case", D.KAT_DISTINCT["cases"], ids=lambda c: c["variant"])
def test_kat_inter_segment_distinct_count(sv, case):
    """InterSegmentAggregationSingleValueQueriesTest.java:176-195: values and the full statistics tuple."""
    t, h = sv
    q = parse_query(case["query"])
    if case["filter"]:
        q.filter = QueryContext.filter_from_json(K.KAT["query_filter"])
    if case["group_by"]:
        q.group_by = [D.KAT_DISTINCT["group_by_column"]]
    with t.plan([h] * 4, q) as p:
        p.execute()
        r = p.finalize()
        assert p.group_path() in ("lds", "global")
        assert p.scan_geometry()["variant"] in (SPARSE, DENSE)
    rows = r.values
    assert all(isinstance(x, int) for row in rows for x in row)
    top = [max(row[a] for row in rows) for a in range(2)]  # PQL: the top group per function
    assert [str(x) for x in top] == case["values"]
    assert tuple(r.stats.as_tuple()[:4]) == tuple(case["stats"])


# ------------------------------------------------------------------------------------------------ numpy parity
@pytest.mark.parametrize("group_by", [["g1"], ["g1", "g2"]], ids=["one_key", "two_keys"])
@pytest.mark.parametrize("f_below", [None, 150], ids=["all", "f15"])
def test_parity_int_and_string(data, group_by, f_below):
    t, hs, segs, allc = data
    q = parse_query("SELECT DISTINCTCOUNT(v), DISTINCTCOUNT(s) FROM t%s GROUP BY %s" % (_where(f_below), ", ".join(group_by)))
    got, stats, path, variant = _run(t, hs, q)
    m = _mask(allc, f_below)
    exp = D.distinct_counts([allc[c] for c in group_by], [allc["v"], allc["s"]], m)
    assert got == exp
    assert path == "lds" and variant == (DENSE if f_below is None else SPARSE)
    # numEntriesScannedPostFilter: docs x distinct group-by and aggregation columns
    assert stats[0] == int(m.sum()) and stats[2] == int(m.sum()) * (len(group_by) + 2)


@pytest.mark.parametrize("card", [1, 64, 65, 130])
def test_word_boundaries(oracle, gpu_lib, card):
    """Global cardinalities at the bitmap's word boundaries; the two local dictionaries overlap partly."""
    rng = np.random.default_rng(card)
    schema = [("g", "INT"), ("v", "INT")]
    a_hi, b_lo = max(1, (2 * card) // 5), (3 * card) // 10
    cols = []
    for n, (lo, hi) in zip(DOCS, ((0, a_hi), (b_lo, card))):
        v = rng.integers(lo, hi, n)
        v[:min(hi - lo, n)] = np.arange(lo, hi)[:n]
        cols.append({"g": rng.integers(0, 3, n), "v": v})
    with GpuTable(schema) as t:
        hs = [t.pin_segment(oracle.make_segment(schema, c)) for c in cols]
        assert len(t.dictionary("v")) == card
        got, _, path, variant = _run(t, hs, parse_query("SELECT DISTINCTCOUNT(v) FROM t GROUP BY g"))
        g = np.concatenate([c["g"] for c in cols])
        v = np.concatenate([c["v"] for c in cols])
        assert got == D.distinct_counts([g], [v], np.ones(len(g), dtype=bool))
        assert path == "lds" and variant == DENSE
        # the whole set, every bit of the last word included
        tot = t.execute_aggregation(hs, parse_query("SELECT DISTINCTCOUNT(v) FROM t"))
        assert tot.values == [len(set(v.tolist()))]


def test_distinct_column_is_a_group_by_column(data):
    t, hs, segs, allc = data
    got, _, _, variant = _run(t, hs, parse_query("SELECT DISTINCTCOUNT(v), COUNT(*) FROM t GROUP BY v"))
    vals, cnts = np.unique(allc["v"], return_counts=True)
    assert got == {(int(k),): [1, int(c)] for k, c in zip(vals, cnts)}
    assert variant == DENSE


def test_beside_other_aggregations(oracle, data):
    """Two DISTINCTCOUNTs beside SUM, AVG and MIN (one of them over the distinct column): the others equal the
    oracle's for the query without the distinct functions; groups without a match are absent."""
    t, hs, segs, allc = data
    where = " WHERE f < 150 AND g1 <> 3"
    q = parse_query("SELECT SUM(m), DISTINCTCOUNT(v), AVG(md), MIN(v), DISTINCTCOUNT(s) FROM t%s GROUP BY g1, g2" % where)
    q0 = parse_query("SELECT SUM(m), AVG(md), MIN(v) FROM t%s GROUP BY g1, g2" % where)
    got, stats, path, variant = _run(t, hs, q)
    o = oracle.run_groupby(SCHEMA, segs, q0)
    m = (allc["f"] < 150) & (allc["g1"] != 3)
    exp = D.distinct_counts([allc["g1"], allc["g2"]], [allc["v"], allc["s"]], m)
    assert set(got) == set(exp) == set(o.groups)
    assert not any(k[0] == 3 for k in got)
    for k, row in got.items():
        assert [row[1], row[4]] == exp[k]
        assert row[0] == o.groups[k][0] and row[3] == o.groups[k][2]
        assert row[2].count == o.groups[k][1].count and row[2].sum == pytest.approx(o.groups[k][1].sum, rel=1e-9)
    assert stats[0] == o.stats[0] == int(m.sum()) and stats[1] == o.stats[1]
    assert variant == SPARSE


# ------------------------------------------------------------------------------------------------ aggregation paths
@pytest.mark.parametrize("f_below,dense_sel,variant", [(10, 0.25, SPARSE), (150, 0.25, SPARSE), (150, 0.1, DENSE),
                                                       (None, 0.25, DENSE)],
                         ids=["queue_1pct", "batch_15pct", "dense_instance_15pct", "dense_all"])
def test_each_aggregation_path(data, f_below, dense_sel, variant):
    """~1 %: the wave queue (flush_wave_queue); ~15 %: lanes with more than 2 matches (aggregate_batch), in the sparse
    and -- dense_selectivity lowered -- the dense instance, whose wave-tiles past 256 matches decode whole groups;
    no filter: aggregate_group on every full tile."""
    t, hs, segs, allc = data
    q = parse_query("SELECT COUNT(*), DISTINCTCOUNT(v) FROM t%s GROUP BY g1, g2" % _where(f_below))
    m = _mask(allc, f_below)
    if f_below == 150:  # some lane's 32-doc group holds more than 2 matches
        assert np.add.reduceat(m[:8192].astype(int), np.arange(0, 8192, 32)).max() > 2
    t.set_config(dense_selectivity=dense_sel)
    try:
        got, _, path, v = _run(t, hs, q)
    finally:
        t.reset_config()
    # (the docs of a group are distinct: the first count is COUNT(*))
    assert got == D.distinct_counts([allc["g1"], allc["g2"]], [np.arange(len(m)), allc["v"]], m)
    assert path == "lds" and v == variant


def test_lds_and_global_tables_agree(data):
    """lds_table_kb at its smallest value (1 KB): the 35-key table of 4 rows (1120 bytes) no longer fits, the plan takes
    global atomics."""
    t, hs, segs, allc = data
    out = {}
    for f_below in (None, 150):
        q = parse_query("SELECT COUNT(*), DISTINCTCOUNT(v), DISTINCTCOUNT(s), SUM(m) FROM t%s GROUP BY g1, g2"
                        % _where(f_below))
        lds, _, p0, v0 = _run(t, hs, q)
        t.set_config(lds_table_kb=1)
        try:
            glb, _, p1, v1 = _run(t, hs, q)
        finally:
            t.reset_config()
        assert (p0, p1) == ("lds", "global") and v0 == v1 == (DENSE if f_below is None else SPARSE)
        assert lds == glb
        m = _mask(allc, f_below)
        exp = D.distinct_counts([allc["g1"], allc["g2"]], [allc["v"], allc["s"]], m)
        assert {k: v[1:3] for k, v in glb.items()} == exp
        out[f_below] = glb
    assert out[None] != out[150]


def test_aggregation_only(data):
    """G == 1: with a filter, without one (answered as from the dictionaries: nothing scanned post filter), and with
    no doc matched (the function's default, 0)."""
    t, hs, segs, allc = data
    for f_below in (None, 150, 10):
        q = parse_query("SELECT DISTINCTCOUNT(v), DISTINCT_COUNT(s), MAX(v) FROM t%s" % _where(f_below))
        with t.plan(hs, q) as p:
            p.execute()
            r = p.finalize()
            assert p.group_path() == "lds" and p.scan_geometry()["variant"] == (DENSE if f_below is None else SPARSE)
        m = _mask(allc, f_below)
        exp = D.distinct_counts([], [allc["v"], allc["s"]], m)[()]
        assert r.values[0][:2] == exp and all(isinstance(x, int) for x in r.values[0][:2])
        # MIN / MAX / DISTINCTCOUNT over match-all segments: as from the dictionaries, nothing scanned post filter
        assert r.stats.as_tuple()[2] == (0 if f_below is None else int(m.sum()) * 2)
    only = t.execute_aggregation(hs, parse_query("SELECT DISTINCTCOUNT(v), DISTINCTCOUNT(s) FROM t"))
    assert only.values == D.distinct_counts([], [allc["v"], allc["s"]], _mask(allc, None))[()]
    assert only.stats.as_tuple()[2] == 0
    none = t.execute_aggregation(hs, parse_query("SELECT DISTINCTCOUNT(v), COUNT(*) FROM t WHERE f > 5000"))
    assert none.values == [0, 0] and none.stats.num_docs_scanned == 0


# ------------------------------------------------------------------------------------------------ execution hygiene
def test_reexecution_and_plan_cache(data):
    t, hs, segs, allc = data
    q = parse_query("SELECT DISTINCTCOUNT(v), DISTINCTCOUNT(s) FROM t WHERE f < 400 GROUP BY g1")
    m = allc["f"] < 400
    exp = D.distinct_counts([allc["g1"]], [allc["v"], allc["s"]], m)
    with t.plan(hs, q) as p:
        p.execute()
        p.execute()  # the bitmaps are zeroed per execution
        assert p.finalize().as_dict() == exp
    a = t.execute_groupby(hs, q).as_dict()
    b = t.execute_groupby(hs, q).as_dict()  # a plan-cache hit
    assert a == b == exp


def test_two_plans_in_flight_on_two_streams(data):
    import torch
    t, hs, segs, allc = data
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    q1 = parse_query("SELECT DISTINCTCOUNT(v) FROM t WHERE f < 150 GROUP BY g1, g2")
    q2 = parse_query("SELECT DISTINCTCOUNT(v) FROM t WHERE f >= 150 GROUP BY g1, g2")
    p1 = t.plan_execute(hs, q1, stream=s1.cuda_stream)
    p2 = t.plan_execute(hs, q2, stream=s2.cuda_stream)
    try:
        r2 = p2.finalize(s2.cuda_stream).as_dict()
        r1 = p1.finalize(s1.cuda_stream).as_dict()
    finally:
        p1.close()
        p2.close()
    keys = [allc["g1"], allc["g2"]]
    assert r1 == D.distinct_counts(keys, [allc["v"]], allc["f"] < 150)
    assert r2 == D.distinct_counts(keys, [allc["v"]], allc["f"] >= 150)
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
        with t.plan([h], parse_query("SELECT COUNT(*), DISTINCTCOUNT(m) FROM t GROUP BY d4")) as p:
            p.execute()
            r = p.finalize()
            assert p.star_work()[0] == 0 and p.scan_geometry()["variant"] == DENSE
        exp = D.distinct_counts([cols["d4"]], [cols["m"]], np.ones(6000, dtype=bool))
        assert {k: v[1] for k, v in r.as_dict().items()} == {k: v[0] for k, v in exp.items()}
        assert r.stats.num_docs_scanned == 6000


def test_order_by_distinct_count_desc_limit(data):
    t, hs, segs, allc = data
    q = parse_query("SELECT g1, g2, DISTINCTCOUNT(v) FROM t WHERE f < 30 GROUP BY g1, g2 "
                    "ORDER BY DISTINCTCOUNT(v) DESC LIMIT 3")
    q.min_server_group_trim_size = 1  # the server keeps max(limit * 5, 1) = 15 groups
    top = t.execute_groupby(hs, q).trim_sql()
    exp = D.distinct_counts([allc["g1"], allc["g2"]], [allc["v"]], allc["f"] < 30)
    # descending count; ties by the composite key (the last group-by column the most significant)
    order = sorted(exp.items(), key=lambda kv: (-kv[1][0], kv[0][1], kv[0][0]))
    assert len(top) == 15
    assert top.keys[:3] == [k for k, _ in order[:3]]
    assert [v[0] for v in top.values[:3]] == [v[0] for _, v in order[:3]]
    assert len({v[0] for _, v in order}) < len(order)  # the data has ties


# ------------------------------------------------------------------------------------------------ declined shapes
def _declined(fn):
    with pytest.raises(L.UnsupportedQueryError) as e:
        fn()
    assert "DISTINCTCOUNT" in str(e.value), str(e.value)


def test_declined_bitmap_cap(oracle, gpu_lib):
    """1024 x 1024 keys x ceil(16384 / 64) words x 8 bytes = 2 GiB of bitmap, above the 1 GiB cap."""
    schema = [("a", "INT"), ("b", "INT"), ("v", "INT")]
    n = 16384
    cols = {"a": np.arange(n) % 1024, "b": (np.arange(n) // 16) % 1024, "v": np.arange(n)}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        _declined(lambda: t.plan([h], parse_query("SELECT DISTINCTCOUNT(v) FROM t GROUP BY a, b", num_groups_limit=10 ** 9)))
        # half the keys fit
        with t.plan([h], parse_query("SELECT DISTINCTCOUNT(b) FROM t GROUP BY a", num_groups_limit=10 ** 9)) as p:
            assert p.group_path() == "lds"


def test_declined_hash_key_space(oracle, gpu_lib):
    """9000 x 9000 keys: past every dense table."""
    schema = [("h1", "INT"), ("h2", "INT"), ("v", "INT")]
    n = 9000
    cols = {"h1": np.arange(n), "h2": np.arange(n)[::-1].copy(), "v": np.arange(n) % 50}
    with GpuTable(schema) as t:
        h = t.pin_segment(oracle.make_segment(schema, cols))
        with t.plan([h], parse_query("SELECT COUNT(*) FROM t GROUP BY h1, h2", num_groups_limit=10 ** 9)) as p:
            assert p.group_path() in ("hash", "hash_partitioned")
        _declined(lambda: t.plan([h], parse_query("SELECT DISTINCTCOUNT(v) FROM t GROUP BY h1, h2",
                                                  num_groups_limit=10 ** 9)))


def test_declined_array_map_stages(sv):
    t, h = sv
    case = K.KAT["inner_segment_group_by"][3]  # 9 group-by columns: the cardinality product overflows a long
    q = QueryContext(case["group_by"], [("DISTINCTCOUNT", "column1")], None, num_groups_limit=10 ** 9)
    _declined(lambda: t.plan([h], q))


def test_declined_num_groups_limit(sv):
    t, h = sv
    q = QueryContext(["column1"], [("COUNT", "*"), ("DISTINCTCOUNT", "column3")], None, num_groups_limit=1000)
    _declined(lambda: t.plan([h], q))
    _declined(lambda: t.execute_groupby([h], q))


def test_declined_raw_column_and_exact_fp_sum(oracle, data):
    from pinot_amd.segment import SegmentBuffers, build_raw_column
    t, hs, segs, allc = data
    q = parse_query("SELECT SUM(md), DISTINCTCOUNT(v) FROM t GROUP BY g1", exact_fp_sum=True)
    _declined(lambda: t.plan(hs, q))
    schema = [("g", "INT"), ("r", "LONG")]
    vals = np.arange(64, dtype=np.int64) * 3
    base = oracle.make_segment([("g", "INT")], {"g": np.arange(64) % 4})
    cols = {**base.columns, "r": build_raw_column("LONG", vals.tolist(), 2)}
    with GpuTable(schema) as t2:
        h = t2.pin_segment(SegmentBuffers(64, cols))
        assert t2.execute_groupby([h], parse_query("SELECT SUM(r) FROM t GROUP BY g")).as_dict()[(0,)] == [int(vals[::4].sum())]
        _declined(lambda: t2.plan([h], parse_query("SELECT DISTINCTCOUNT(r) FROM t GROUP BY g")))


def test_declined_external_merges(data):
    """finalize_range, an external d_table (execute, finalize, create_execute), exchange_counts, datatable()."""
    import torch
    t, hs, segs, allc = data
    q = parse_query("SELECT COUNT(*), DISTINCTCOUNT(v) FROM t GROUP BY g1, g2")
    d = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    _declined(lambda: t.plan_execute(hs, q, d_table=d.data_ptr()))
    with t.plan(hs, q) as p:
        ns, nk, kinds = p.layout()
        assert (ns, nk, kinds) == (2, 35, [L.SLOT_COUNT, L.SLOT_SUM_I64])  # an int64 row to everything downstream
        _declined(lambda: p.execute(None, d.data_ptr()))
        p.execute()
        _declined(lambda: p.finalize(None, d.data_ptr()))
        _declined(lambda: p.finalize_range(None, d.data_ptr(), 0, nk))
        _declined(lambda: p.exchange_counts(None, 2))
        r = p.finalize()
        _declined(r.datatable)
        exp = D.distinct_counts([allc["g1"], allc["g2"]], [np.arange(len(allc["f"])), allc["v"]], _mask(allc, None))
        assert r.as_dict() == exp  # (the docs of a group are distinct: the first count is COUNT(*))
