"""Fixed-point FLOAT / DOUBLE sums (exact_fp_sum=True) on the partitioned pipelines: agreed plans
(GpuTable.plan(..., fp_sum_ranges=...), pgpu_plan_create_agreed) keep the radix-partitioned (K8a-K8d) and the
hash-partitioned (K8a-K8h) group-by, whose record passes carry the operand's double as one stream and whose aggregate
kernels' FX instances (part_aggregate_fx_kernel, part_hash_aggregate_fx_kernel) split it into its W digits where the
records are accumulated.  One process; the agreed ranges are the table's own (GpuTable.fp_sum_ranges), so the formats
are those of the plain plan, which keeps the scan kernel's global / hash table (tests/test_fp_sum_exact_gpu.py pins
that): the two paths must give the same bits, and both must equal math.fsum per group.

Data and helpers are those of tests/test_fp_sum_exact_gpu.py.  Dense: 10^6 keys x 6 (W = 2) or 7 (W = 3) slots, a 48 /
56 MB table, past the 32 MB from which a dense table is radix-partitioned, over
  scattered  that file's data set at 1, 33 and 8193 docs per segment: a1 and a2 are uniform over 1000 values each, so
             its 24 579 docs fall into 24 259 groups -- records all over the partitions, but one operand per group:
             the order of a sum cannot matter there, and assert_order_matters cannot hold on it (the doc-order sums
             equal math.fsum in 24 259 of 24 259 groups);
  clustered  the same rows with a1 and a2 drawn from 12 values each, spread over the 1000: 144 groups of about 170
             docs in the same key space, on which the CPU precondition is asserted before the GPU is touched.
Hashed: about 1 600 groups in a key space of 8.1e7 (past 2^26, below 2^31), under the default shape and under a 4 KB
LDS table without partition bits -- 256 entries (the smallest table K8h has) for 1 600 groups, so K8h takes several
rounds and splits again the records it wrote back.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd import _lib as L
from pinot_amd.query import parse_query
from test_fp_sum_exact_gpu import (Data, _columns, assert_bit_equal, assert_exact_w2, assert_order_matters, bits,
                                   data, fsums)  # noqa: F401 -- `data` is the module-scoped fixture

pytestmark = pytest.mark.gpu

DENSE_TAIL = "COUNT(*), MIN(f), MAX(f), SUM(f) FROM t GROUP BY a1, a2"
DENSE_KEYS = ("a1", "a2")


def run(d, sql, agreed=True, **cfg):
    """(values by key, group path, formats per aggregation) of one execution of an agreed (own ranges) or plain plan."""
    q = parse_query(sql, num_groups_limit=10 ** 9, exact_fp_sum=True)
    if cfg:
        d.t.set_config(**cfg)
    try:
        ranges = d.t.fp_sum_ranges(d.hs, q) if agreed else None
        with d.t.plan_execute(d.hs, q, fp_sum_ranges=ranges) as p:
            r = p.finalize()
            fm = [p.fp_sum_format(a) for a in range(len(q.aggregations))]
            return r.as_dict(), p.group_path(), fm
    finally:
        if cfg:
            d.t.reset_config()


def same_bits(a, b, agg=0, sum_of=lambda v: v):
    assert set(a) == set(b)
    bad = [k for k in a if bits(sum_of(a[k][agg])) != bits(sum_of(b[k][agg]))]
    assert not bad, "%d of %d groups differ between the paths, e.g. %s" % (len(bad), len(a), bad[:3])


# ------------------------------------------------------------------------------------------------------- dense
CLUSTER_N = 8193


@pytest.fixture(scope="module")
def dense(oracle, data):
    """(set, docs per segment) -> its Data."""
    own = {}

    def get(which, n):
        if which == "scattered":
            return data(n)
        if n not in own:
            cols = []
            for s in range(3):
                c = _columns(n, s)
                rng = np.random.default_rng(57 + s)
                for k in DENSE_KEYS:
                    c[k] = rng.integers(0, 12, n).astype(np.int64) * 83 + 5
                cols.append(c)
            own[n] = Data(oracle, cols)
        return own[n]
    yield get
    for d in own.values():
        d.close()


DENSE_SETS = [("scattered", 1), ("scattered", 33), ("scattered", 8193), ("clustered", CLUSTER_N)]
DENSE_IDS = ["%s-%d" % s for s in DENSE_SETS]


def precondition(which, groups):
    if which == "clustered":
        assert 100 <= len(groups) <= 144
        assert_order_matters(groups)


@pytest.mark.parametrize("which,n", DENSE_SETS, ids=DENSE_IDS)
def test_dense_sum_is_bit_equal_to_fsum(dense, which, n):
    d = dense(which, n)
    groups = d.groups(DENSE_KEYS, "x")
    precondition(which, groups)
    got, path, fm = run(d, "SELECT SUM(x), " + DENSE_TAIL)
    assert path == "partitioned", path
    assert_exact_w2(fm[0])
    assert all(f["mode"] == "none" for f in fm[1:]), fm
    assert_bit_equal(got, fsums(groups))
    f = d.groups(DENSE_KEYS, "f")
    for k, v in groups.items():  # the other slots of the records: COUNT, MIN, MAX and the integer SUM
        assert got[k][1:] == [len(v), float(f[k].min()), float(f[k].max()), float(f[k].sum())], k
    # path independence: the plain plan (global table, the scan kernel's split) has the same format and the same bits
    plain, ppath, pfm = run(d, "SELECT SUM(x), " + DENSE_TAIL, agreed=False)
    assert ppath == "global" and pfm == fm, (ppath, pfm, fm)
    same_bits(got, plain)


@pytest.mark.parametrize("which,n", DENSE_SETS[1:], ids=DENSE_IDS[1:])
def test_dense_avg_is_bit_equal_to_fsum(dense, which, n):
    d = dense(which, n)
    groups = d.groups(DENSE_KEYS, "x")
    precondition(which, groups)
    got, path, fm = run(d, "SELECT AVG(x), " + DENSE_TAIL)
    assert path == "partitioned", path
    assert_exact_w2(fm[0])
    assert_bit_equal(got, fsums(groups), sum_of=lambda pair: pair.sum)
    for k, v in groups.items():
        assert got[k][0].count == len(v) == got[k][1]


@pytest.mark.parametrize("which,n", DENSE_SETS[2:], ids=DENSE_IDS[2:])
def test_dense_three_digits(dense, which, n):
    d = dense(which, n)
    groups = d.groups(DENSE_KEYS, "w")
    precondition(which, groups)
    got, path, fm = run(d, "SELECT SUM(w), " + DENSE_TAIL)
    assert path == "partitioned", path
    assert fm[0]["mode"] == "exact" and fm[0]["W"] == 3 and fm[0]["E"] == 10, fm
    assert fm[0]["K"] == 62 - (3 * n).bit_length() - 1, fm
    assert_bit_equal(got, fsums(groups))


def test_dense_two_columns_share_one_pass(dense):
    """SUM(x) (W = 2) and SUM(w) (W = 3) in one query: two streams, five digit slots, 9 slots in all."""
    d = dense("clustered", CLUSTER_N)
    got, path, fm = run(d, "SELECT SUM(x), SUM(w), " + DENSE_TAIL)
    assert path == "partitioned", path
    assert fm[0]["W"] == 2 and fm[1]["W"] == 3, fm
    assert_bit_equal(got, fsums(d.groups(DENSE_KEYS, "x")), agg=0)
    assert_bit_equal(got, fsums(d.groups(DENSE_KEYS, "w")), agg=1)


@pytest.mark.parametrize("which,n", DENSE_SETS[1:], ids=DENSE_IDS[1:])
def test_dense_quantised_format_matches_its_definition(dense, which, n):
    """The truncated-operand reference of test_quantised_format_matches_its_definition, on the partitioned path."""
    d = dense(which, n)
    groups = d.groups(DENSE_KEYS, "z")
    got, path, fms = run(d, "SELECT SUM(z), " + DENSE_TAIL)
    assert path == "partitioned", path
    fm = fms[0]
    assert fm["mode"] == "quantised" and fm["W"] == 3 and fm["E"] == 61, fm
    q = fm["E"] - fm["W"] * fm["K"]
    scale = Fraction(2) ** -q if q < 0 else Fraction(1, 2 ** q)
    want = {}
    for k, v in groups.items():
        total = sum(int(Fraction(x) * scale) for x in v.tolist())  # int(): truncation toward zero
        want[k] = float(Fraction(total) / scale)                   # int / int: correctly rounded
    assert_bit_equal(got, want)


# ------------------------------------------------------------------------------------------------------ hashed
HASH_N = 20000  # about 37 docs per group: the doc-order sum differs from math.fsum in two thirds of the groups


@pytest.fixture(scope="module")
def hashed(oracle, gpu_lib):
    """The exact data set with 40 values of each of h1 and h2: about 1 600 groups in the 9000 x 9000 key space."""
    cols = []
    for s in range(3):
        c = _columns(HASH_N, s)
        rng = np.random.default_rng(31 + s)
        for k in ("h1", "h2"):
            c[k] = rng.integers(0, 40, HASH_N).astype(np.int64) * 200 + 7
        cols.append(c)
    d = Data(oracle, cols)
    yield d
    d.close()


@pytest.mark.parametrize("cfg", [{}, {"hash_partition_bits": 0, "hash_partition_lds_kb": 4}], ids=["default", "rounds"])
def test_hashed_sum_is_bit_equal_to_fsum(hashed, cfg):
    d = hashed
    groups = d.groups(("h1", "h2"), "x")
    assert 1500 <= len(groups) <= 1600 and 2 ** 26 < 9000 * 9000 < 2 ** 31
    assert_order_matters(groups)  # before the GPU is touched
    if cfg:  # 3 slots: entries of 8 x 3 + 4 bytes, so a 4 KB table would hold 146; K8h's smallest has 256
        assert 4096 // (8 * 3 + 4) < 256 < len(groups) / 5
    got, path, fm = run(d, "SELECT SUM(x), COUNT(*) FROM t GROUP BY h1, h2", **cfg)
    assert path == "hash_partitioned", path
    assert_exact_w2(fm[0])
    assert_bit_equal(got, fsums(groups))
    for k, v in groups.items():
        assert got[k][1] == len(v)
    plain, ppath, pfm = run(d, "SELECT SUM(x), COUNT(*) FROM t GROUP BY h1, h2", agreed=False, **cfg)
    assert ppath == "hash" and pfm == fm, (ppath, pfm, fm)
    same_bits(got, plain)


# ---------------------------------------------------------------------------------------------------- planning
def test_own_ranges_are_what_the_plain_plan_reads(data):
    d = data(8193)
    q = parse_query("SELECT SUM(x), COUNT(*), SUM(f), AVG(z), MIN(x) FROM t GROUP BY d", exact_fp_sum=True)
    r = [x.as_tuple() for x in d.t.fp_sum_ranges(d.hs, q)]
    docs = 3 * 8193
    assert r[0] == (1, 1, 1, 55, -30, docs, 0.0)
    assert r[1] == (0, 0, 0, 0, 0, 0, 0.0) and r[4] == (0, 0, 0, 0, 0, 0, 0.0)
    # an integer column: its values as doubles, and the bound int_sum_fits compares with 2^62
    fmax = [int(c["f"].max()) for c in d.cols]
    assert r[2][:3] == (1, 1, 1) and r[2][5] == docs and r[2][6] == float(sum(8193 * m for m in fmax))
    assert r[3][:4] == (1, 1, 1, 61) and r[3][4] == -132
    with d.t.plan(d.hs, q) as plain, d.t.plan(d.hs, q, fp_sum_ranges=d.t.fp_sum_ranges(d.hs, q)) as agreed:
        for a in range(5):
            assert plain.fp_sum_format(a) == agreed.fp_sum_format(a)
        assert plain.layout() == agreed.layout()


def test_agreed_ranges_decide_slots_and_formats(data):
    """More docs and a wider range than the table's own, as other ranks would add: K shrinks with the agreed docs, E
    and L are the agreed ones; an integer bound past 2^62 turns the int64 slot into digits on this rank too."""
    d = data(33)
    q = parse_query("SELECT SUM(x), SUM(f) FROM t GROUP BY d", exact_fp_sum=True)
    own = [x.as_tuple() for x in d.t.fp_sum_ranges(d.hs, q)]
    wide = [(1, 1, 1, 60, -32, 10 ** 6, 0.0), own[1][:6] + (2.0 ** 62,)]
    with d.t.plan(d.hs, q, fp_sum_ranges=wide) as p:
        assert p.fp_sum_format(0) == {"mode": "exact", "E": 60, "K": 62 - (10 ** 6).bit_length() - 1, "W": 3}
        assert p.fp_sum_format(1)["mode"] == "exact" and p.fp_sum_format(1)["W"] == 2
        assert p.layout()[0] == 1 + 3 + 2
        p.execute()
        got = p.finalize().as_dict()
    assert_bit_equal(got, fsums(d.groups(("d",), "x")), agg=0)
    f = d.groups(("d",), "f")
    assert {k: v[1] for k, v in got.items()} == {k: float(v.sum()) for k, v in f.items()}
    with d.t.plan(d.hs, q, fp_sum_ranges=[own[0], own[1][:6] + (2.0 ** 62 - 1024.0,)]) as p:
        assert p.fp_sum_format(1)["mode"] == "none" and p.layout()[0] == 1 + 2 + 1
    with d.t.plan(d.hs, q, fp_sum_ranges=[own[0][:2] + (0,) + own[0][3:], own[1]]) as p:  # a non-finite rank
        assert p.fp_sum_format(0)["mode"] == "none" and p.layout()[2][1] == L.SLOT_SUM_F64


def test_agreed_plan_needs_the_option_and_matching_ranges(data):
    d = data(33)
    q = parse_query("SELECT SUM(x), COUNT(*) FROM t GROUP BY d", exact_fp_sum=True)
    own = d.t.fp_sum_ranges(d.hs, q)
    with pytest.raises(L.PinotGpuError) as e:
        d.t.plan(d.hs, parse_query("SELECT SUM(x), COUNT(*) FROM t GROUP BY d"), fp_sum_ranges=own)
    assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and "PGPU_OPT_EXACT_FP_SUM" in e.value.message
    with pytest.raises(L.PinotGpuError) as e:
        d.t.plan(d.hs, q, fp_sum_ranges=own[::-1])
    assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and "aggregation 0" in e.value.message
    assert math.isfinite(own[0].int_sum_bound)
