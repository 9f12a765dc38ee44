"""Bit-reproducible FLOAT / DOUBLE SUM / AVG (QueryContext(exact_fp_sum=True), PGPU_OPT_EXACT_FP_SUM) on the GPU.

Every operand is split into W fixed-point digits that are summed as integers (pinot_amd/csrc/fx_sum.h), so the sum no
longer depends on the order the scan's atomics land in.  In an exact format the result is the correctly rounded exact
sum, which is what math.fsum returns: the exact cases compare bit for bit with math.fsum per group, not with the
oracle's 1e-9 -- their operands cancel, so a doc-order float64 sum legitimately differs by more.

The exact cases share one data set per segment size n in {1, 33, 8193, 70001}: 3 segments of n docs with different
dictionaries -- odd multiples of 4 near +-2^54 (segment 0: E = 55 comes from it), near 2^53 and 2^52, against odd
multiples of 2^-20, 2^-25 and 2^-30 (segment 2: L = -30 comes from it), in random signs so that the large operands
partly cancel.  E - L = 85 <= 2 K for up to 2^18 - 1 docs (K = 62 - bit_length(docs) - 1 >= 43), so W = 2 is exact.
Before the GPU is touched each case with >= 8193 docs asserts on the CPU that the doc-order float64 sum differs from
math.fsum in more than half of its groups: a path that is not exact cannot pass by luck.

Each case asserts through Plan.group_path / Plan.scan_geometry()["variant"] that it ran in the accumulator mode and
scan instance it names.  The star-tree case sums the pre-aggregated doubles of the star-tree documents the traversal
selects (those are the operands the star path reads); its reference is math.fsum over the same documents.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import startree_common as SC
from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import parse_query
from pinot_amd.segment import SegmentBuffers, build_raw_column
from pinot_amd.startree import StarTree
from pinot_amd.workloads import double_table

pytestmark = pytest.mark.gpu

SIZES = (1, 33, 8193, 70001)
# d: 64 groups (an LDS table of 64 x 3 slots is 1.5 KB: past lds_table_kb = 1); h1 x h2: a key space of 8.1e7, past
# every dense table (2^26), so hash mode -- sparse: the docs use 8 values of each; a1 x a2: 10^6 keys; f: the filter
# column; x: the exact data set, r: the same values raw;
# w: the W = 3 dictionary; z: operands spanning 2^60 .. 2^-80 (quantised); v: x with an infinity in one dictionary
SCHEMA = [("d", "INT"), ("h1", "INT"), ("h2", "INT"), ("a1", "INT"), ("a2", "INT"), ("f", "INT"), ("x", "DOUBLE"),
          ("r", "DOUBLE"), ("w", "DOUBLE"), ("z", "DOUBLE"), ("v", "DOUBLE")]
CARDS = {"d": 64, "h1": 9000, "h2": 9000, "a1": 1000, "a2": 1000, "f": 1000}
VARIANT_FX_SPARSE, VARIANT_FX_DENSE = 6, 7


def _exact_values(rng, n, seg):
    base = (2.0 ** 54, 2.0 ** 53, 2.0 ** 52)[seg % 3]
    small = (2.0 ** -20, 2.0 ** -25, 2.0 ** -30)[seg % 3]
    kind = rng.integers(0, 5, n)
    big = base + 4.0 * (2 * rng.integers(0, 500, n) + 1)
    x = np.where(kind < 2, big, np.where(kind < 4, -big, (2 * rng.integers(0, 100000, n) + 1) * small))
    if n >= 3:  # every segment holds its largest and its smallest kind of operand, whatever the draw
        x[0], x[1], x[2] = base + 4.0, -(base + 12.0), 3 * small
    return x


W3_DICT = np.concatenate([double_table(2000, 3, 0.0, 1000.0), double_table(2000, 4, 0.0, 1000.0) * 2.0 ** -40])


def _columns(n, seg):
    rng = np.random.default_rng(1000 * seg + n)
    cols = {c: rng.integers(0, card, n).astype(np.int64) for c, card in CARDS.items()}
    for c in ("h1", "h2"):
        cols[c] = rng.integers(0, 8, n).astype(np.int64) * 1000 + 7
    cols["x"] = _exact_values(rng, n, seg)
    cols["w"] = W3_DICT[rng.integers(0, len(W3_DICT), n)]
    mant = (rng.integers(0, 2 ** 52, n) | 1).astype(np.float64) + 2.0 ** 52
    cols["z"] = np.ldexp(mant, rng.integers(-80 - 52, 60 - 52 + 1, n).astype(np.int32)) * rng.choice([-1.0, 1.0], n)
    if n >= 2:  # both ends of the span in every segment: E = 61, lowest bit 2^-132
        cols["z"][0], cols["z"][1] = math.ldexp(2.0 ** 52 + 1, 8), -math.ldexp(2.0 ** 52 + 1, -132)
    cols["v"] = cols["x"].copy()
    if seg == 1:
        cols["v"][n // 2] = math.inf
    return cols


class Data:
    """A table of len(cols) segments, pinned, with the key columns' global dictionaries at their full cardinality
    (so that a table of 3 docs plans the same key spaces as one of 210 003)."""

    def __init__(self, oracle, seg_cols):
        self.cols = seg_cols
        self.segs = []
        for c in seg_cols:
            base = oracle.make_segment([s for s in SCHEMA if s[0] != "r"], c)
            raw = {"r": build_raw_column("DOUBLE", c["x"].tolist())}
            self.segs.append(SegmentBuffers(len(c["x"]), {**base.columns, **raw}))
        self.t = GpuTable(SCHEMA)
        for c, card in CARDS.items():
            self.t.add_dictionary_values(c, list(range(card)))
        self.hs = [self.t.pin_segment(s) for s in self.segs]
        self.all = {k: np.concatenate([c[k] for c in seg_cols]) for k in seg_cols[0]}
        self.all["r"] = self.all["x"]
        self._groups = {}

    def groups(self, keys, col, where=None):
        """{key tuple: the group's operands in doc order}; computed once per (keys, col, filter)."""
        ck = (tuple(keys), col, where)
        if ck not in self._groups:
            a = self.all
            sel = np.ones(len(a[col]), dtype=bool) if where is None else a[where[0]] < where[1]
            vals = a[col][sel]
            if not keys:
                out = {(): vals} if len(vals) else {}
            else:
                km = np.stack([a[k][sel] for k in keys], axis=1)
                order = np.lexsort(km.T[::-1])
                km, vals = km[order], vals[order]  # lexsort is stable: doc order inside a group
                cut = np.nonzero(np.any(km[1:] != km[:-1], axis=1))[0] + 1
                out = {tuple(int(v) for v in km[s]): vals[s:e]
                       for s, e in zip(np.r_[0, cut], np.r_[cut, len(vals)]) if e > s}
            self._groups[ck] = out
        return self._groups[ck]

    def close(self):
        self.t.close()


_DATA = {}


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    def get(n):
        if n not in _DATA:
            _DATA[n] = Data(oracle, [_columns(n, s) for s in range(3)])
        return _DATA[n]
    yield get
    for d in _DATA.values():
        d.close()
    _DATA.clear()


def fsums(groups):
    return {k: math.fsum(v.tolist()) for k, v in groups.items()}


def assert_order_matters(groups):
    """The CPU precondition: the doc-order float64 sum (np.cumsum adds sequentially) is not the exact sum in more than
    half of the groups."""
    differ = sum(1 for v in groups.values() if float(np.cumsum(v)[-1]) != math.fsum(v.tolist()))
    assert differ * 2 > len(groups), "doc-order sums equal math.fsum in %d of %d groups" % (len(groups) - differ,
                                                                                          len(groups))


def run(d, sql, exact=True, **cfg):
    """(values by key, group path, scan instance, formats per aggregation) of one execution."""
    q = parse_query(sql, num_groups_limit=10 ** 9, exact_fp_sum=exact)
    if cfg:
        d.t.set_config(**cfg)
    try:
        with d.t.plan_execute(d.hs, q) as p:
            r = p.finalize()
            fm = [p.fp_sum_format(a) for a in range(len(q.aggregations))]
            return r.as_dict(), p.group_path(), p.scan_geometry()["variant"], fm
    finally:
        if cfg:
            d.t.reset_config()


def bits(x):
    return float(x).hex()


def assert_bit_equal(got, want, agg=0, sum_of=lambda v: v):
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    bad = [(k, bits(sum_of(got[k][agg])), bits(want[k])) for k in want if bits(sum_of(got[k][agg])) != bits(want[k])]
    assert not bad, "%d of %d groups differ from math.fsum, e.g. %s" % (len(bad), len(want), bad[:3])


def assert_exact_w2(fm):
    assert fm["mode"] == "exact" and fm["W"] == 2 and fm["E"] <= 55 and fm["K"] >= 43, fm


# (case, SQL after SELECT .. FROM t, group-by columns, summed column, filter, config, path, instance (None: either))
CASES = [
    ("aggregation_only", "", (), "x", None, {}, "lds", None),
    ("lds", "GROUP BY d", ("d",), "x", None, {}, "lds", None),
    ("global", "GROUP BY d", ("d",), "x", None, {"lds_table_kb": 1}, "global", None),
    ("hash", "GROUP BY h1, h2", ("h1", "h2"), "x", None, {}, "hash", None),
    ("sparse_instance", "WHERE f < 100 GROUP BY d", ("d",), "x", ("f", 100), {}, "lds", VARIANT_FX_SPARSE),
    ("dense_instance", "GROUP BY d", ("d",), "x", None, {"dense_selectivity": 0.01}, "lds", VARIANT_FX_DENSE),
    ("raw_double", "GROUP BY d", ("d",), "r", None, {}, "lds", None),
]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sum_is_bit_equal_to_fsum(data, case, n):
    name, tail, keys, col, where, cfg, path, variant = case
    d = data(n)
    groups = d.groups(keys, col, where)
    if n >= 8193:
        assert_order_matters(groups)
    got, gpath, gvariant, fm = run(d, "SELECT SUM(%s), COUNT(*) FROM t %s" % (col, tail), **cfg)
    assert gpath == path, "the case ran in %s mode" % gpath
    assert gvariant in (VARIANT_FX_SPARSE, VARIANT_FX_DENSE), gvariant
    # (the selectivity estimate comes from the segments' own dictionaries: over one-entry dictionaries, n = 1, a range
    # predicate is all or nothing, so the sparse case names its instance from 33 docs on)
    if variant is not None and not (name == "sparse_instance" and n == 1):
        assert gvariant == variant, "the case ran scan instance %d" % gvariant
    assert_exact_w2(fm[0])
    assert fm[1] == {"mode": "none", "E": 0, "K": 0, "W": 0}  # COUNT(*)
    assert_bit_equal(got, fsums(groups))
    for k, v in groups.items():
        assert got[k][1] == len(v)


@pytest.mark.parametrize("n", SIZES)
def test_avg_sum_is_bit_equal_to_fsum(data, n):
    d = data(n)
    groups = d.groups(("d",), "x")
    if n >= 8193:
        assert_order_matters(groups)
    got, path, _, fm = run(d, "SELECT AVG(x), SUM(x) FROM t GROUP BY d")
    assert path == "lds"
    assert_exact_w2(fm[0])
    assert fm[1] == fm[0]  # SUM and AVG of a column share the digit slots
    want = fsums(groups)
    assert_bit_equal(got, want, agg=0, sum_of=lambda pair: pair.sum)
    assert_bit_equal(got, want, agg=1)
    for k, v in groups.items():
        assert got[k][0].count == len(v)


# ---------------------------------------------------------------------------------------------------- star-tree
def _star_selected(star, seg, q):
    """(group dictIds, pre-aggregated md) of the star-tree documents the traversal selects for a query without a
    filter: the operands of the star path, as oracle/startree_oracle.py's groupby picks them."""
    gdims = [SC.C4_SPLIT.index(c) for c in q.group_by]
    ranges, remaining = SC.SO.traverse(star["nodes"], {}, set(gdims))
    assert not remaining
    docs = np.concatenate([np.arange(s, e) for s, e in ranges])
    dim_bits = [seg.columns[c].bits_per_element for c in SC.C4_SPLIT]
    ids = [SC.SO.unpack_bits(star["dim_fwd"][g], star["num_docs"], dim_bits[g])[docs] for g in gdims]
    m = SC.C4_PAIRS.index(("SUM", "md"))
    return ids, star["metric_f64"][m][docs]


@pytest.mark.parametrize("n", SIZES)
def test_star_tree_sum_is_bit_equal_to_fsum(oracle, gpu_lib, n):
    rng = np.random.default_rng(77 + n)
    q = parse_query("SELECT SUM(md), COUNT(*) FROM t GROUP BY d3", num_groups_limit=10 ** 9, exact_fp_sum=True)
    segs, stars, groups = [], [], {}
    for s in range(3):
        cols = SC.c4_columns(rng, n, cards=(40, 15, 8, 6))
        cols["md"] = _exact_values(rng, n, s)
        seg = oracle.make_segment(SC.C4_SCHEMA, cols)
        st = StarTree.build(SC.C4_SCHEMA, seg, SC.C4_SPLIT, SC.C4_PAIRS, max_leaf_records=300)
        segs.append(seg)
        stars.append(st)
        (ids,), vals = _star_selected(st.arrays(), seg, q)
        d3 = SC.dictionary_values(seg.columns["d3"])
        for g in np.unique(ids):
            groups.setdefault((int(d3[g]),), []).append(vals[ids == g])
    groups = {k: np.concatenate(v) for k, v in groups.items()}
    if n >= 8193:
        assert_order_matters(groups)
    t = GpuTable(SC.C4_SCHEMA)
    try:
        hs = [t.pin_segment(s) for s in segs]
        for h, st in zip(hs, stars):
            t.attach_startree(h, st)
        with t.plan_execute(hs, q) as p:
            r = p.finalize()
            fm = p.fp_sum_format(0)
            assert p.star_work()[0] == 3, "the plan did not answer its segments from their star-trees"
        assert fm["mode"] == "exact", fm  # pre-aggregated sums reach past 2^55: W is 2 or 3
        assert_bit_equal(r.as_dict(), fsums(groups))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------ shape independence
def test_bits_do_not_depend_on_the_segment_layout_or_the_tile_split(oracle, data):
    """The same rows as 1 segment and as 5 segments, with slot_weight_step 0 and 4.0: identical bits."""
    src = data(70001)
    rows = src.all
    n = len(rows["x"])
    want = fsums(src.groups(("d",), "x"))
    out = []
    for nseg in (1, 5):
        cut = [n * i // nseg for i in range(nseg + 1)]
        d = Data(oracle, [{k: v[a:b] for k, v in rows.items() if k != "r"} for a, b in zip(cut, cut[1:])])
        try:
            for step in (0.0, 4.0):
                got, path, _, fm = run(d, "SELECT SUM(x), COUNT(*) FROM t GROUP BY d", slot_weight_step=step)
                assert path == "lds"
                assert_exact_w2(fm[0])
                out.append({k: bits(v[0]) for k, v in got.items()})
        finally:
            d.close()
    assert all(o == out[0] for o in out[1:])
    assert out[0] == {k: bits(v) for k, v in want.items()}


# ------------------------------------------------------------------------------------------------------- W = 3
@pytest.mark.parametrize("n", (8193, 70001))
def test_three_digits(data, n):
    """A dictionary in the style of C2's `md` (workloads.double_table, U[0, 1000): 53-bit mantissas, E = 10, lowest bits
    near 2^-59), half of it scaled by 2^-40: E - L is about 109, past 2 K (92 at 24 579 docs, 86 at 210 003) and within
    3 K, so the format is exact with W = 3.  (U[0, 1000) alone has E - L of about 69: three digits only from 2^26 docs
    on, where K <= 34 -- no size for a test that runs with every pull request.)"""
    d = data(n)
    groups = d.groups(("d",), "w")
    got, path, _, fm = run(d, "SELECT SUM(w) FROM t GROUP BY d")
    assert path == "lds"
    assert fm[0]["mode"] == "exact" and fm[0]["W"] == 3 and fm[0]["E"] == 10, fm
    assert fm[0]["K"] == 62 - (3 * n).bit_length() - 1, fm
    assert_bit_equal(got, fsums(groups))


# --------------------------------------------------------------------------------------------------- quantised
@pytest.mark.parametrize("n", (33, 8193))
def test_quantised_format_matches_its_definition(data, n):
    """Operands spanning 2^60 .. 2^-80 do not fit three digits: mode 2.  The result is the correctly rounded sum of
    the operands truncated toward zero to multiples of 2^(E - W K), evaluated here in Python integers from the
    (E, K, W) the plan reports; two executions and two accumulator modes give the same bits."""
    d = data(n)
    groups = d.groups(("d",), "z")
    runs = [run(d, "SELECT SUM(z) FROM t GROUP BY d"), run(d, "SELECT SUM(z) FROM t GROUP BY d"),
            run(d, "SELECT SUM(z) FROM t GROUP BY d", lds_table_kb=1)]
    assert [r[1] for r in runs] == ["lds", "lds", "global"]
    fm = runs[0][3][0]
    assert fm["mode"] == "quantised" and fm["W"] == 3 and fm["E"] == 61, fm
    assert all(r[3][0] == fm for r in runs)
    q = fm["E"] - fm["W"] * fm["K"]
    scale = Fraction(2) ** -q if q < 0 else Fraction(1, 2 ** q)
    want = {}
    for k, v in groups.items():
        total = sum(int(Fraction(x) * scale) for x in v.tolist())  # int(): truncation toward zero
        want[k] = float(Fraction(total) / scale)                   # int / int: correctly rounded
    for r in runs:
        assert_bit_equal(r[0], want)


# -------------------------------------------------------------------------------------------------- non-finite
def test_a_non_finite_dictionary_keeps_the_float_accumulator(data):
    d = data(8193)
    with_opt, path, variant, fm = run(d, "SELECT SUM(v), COUNT(*) FROM t GROUP BY d")
    assert fm[0] == {"mode": "none", "E": 0, "K": 0, "W": 0}
    assert variant not in (VARIANT_FX_SPARSE, VARIANT_FX_DENSE)
    without, _, v0, _ = run(d, "SELECT SUM(v), COUNT(*) FROM t GROUP BY d", exact=False)
    assert v0 == variant
    groups = d.groups(("d",), "v")
    assert set(with_opt) == set(without) == set(groups)
    infs = 0
    for k, vals in groups.items():
        want = math.fsum(vals.tolist()) if np.isfinite(vals).all() else math.inf
        infs += want == math.inf
        for got in (with_opt[k][0], without[k][0]):
            # today's float64 accumulation: the operands cancel from 2^54 down, so the bound is on the operands
            assert got == want or abs(got - want) <= 1e-9 * float(np.abs(vals[np.isfinite(vals)]).sum()), (k, got, want)
    assert infs == 1


# ---------------------------------------------------------------------------------------------------- declines
def test_cross_gpu_entry_points_decline(data):
    from pinot_amd.combine import Communicator, combine_mode
    d = data(33)
    q = parse_query("SELECT SUM(x) FROM t GROUP BY h1, h2", num_groups_limit=10 ** 9, exact_fp_sum=True)
    comm = Communicator(L.COMM_RCCL, Communicator.unique_id(L.COMM_RCCL), 1, 0, 0)
    try:
        with d.t.plan_execute(d.hs, q) as p:
            assert p.group_path() == "hash"
            with pytest.raises(L.UnsupportedQueryError, match="PGPU_OPT_EXACT_FP_SUM"):
                combine_mode(p, comm, 1 << 62)
            with pytest.raises(L.UnsupportedQueryError, match="PGPU_OPT_EXACT_FP_SUM"):
                p.exchange_counts(None, 2)
            assert_bit_equal(p.finalize().as_dict(), fsums(d.groups(("h1", "h2"), "x")))  # the plan is still good
        q = parse_query("SELECT SUM(x) FROM t GROUP BY d", num_groups_limit=10 ** 9, exact_fp_sum=True)
        with d.t.plan_execute(d.hs, q) as p:
            with pytest.raises(L.UnsupportedQueryError, match="PGPU_OPT_EXACT_FP_SUM"):
                combine_mode(p, comm, 1 << 62)
    finally:
        comm.close()


@pytest.mark.parametrize("n", (8193,))
def test_large_key_space_is_not_partitioned(data, n):
    """10^6 keys x 5 slots is a 40 MB table, past the 32 MB from which a dense table is radix-partitioned: without the
    option the plan is, with it (6 slots) it keeps the scan kernel's global table."""
    d = data(n)
    sql = "SELECT SUM(x), COUNT(*), MIN(f), MAX(f), SUM(f) FROM t GROUP BY a1, a2"
    _, plain_path, _, _ = run(d, sql, exact=False)
    assert plain_path == "partitioned", plain_path  # the case is one the partitioned pipeline would take
    got, path, variant, fm = run(d, sql)
    assert path == "global" and variant in (VARIANT_FX_SPARSE, VARIANT_FX_DENSE), (path, variant)
    assert_exact_w2(fm[0])
    assert_bit_equal(got, fsums(d.groups(("a1", "a2"), "x")))


# ------------------------------------------------------------------------------------------------ default path
def test_ordinary_data_agrees_with_the_oracle_with_and_without_the_option(oracle, gpu_lib):
    from test_gpu_parity import assert_same
    rng = np.random.default_rng(5)
    schema = [("d", "INT"), ("f", "INT"), ("md", "DOUBLE")]
    segs = [oracle.make_segment(schema, {"d": rng.integers(0, 40, n), "f": rng.integers(0, 100, n),
                                         "md": rng.uniform(1.0, 1e6, n)}) for n in (8193, 33, 20000)]
    t = GpuTable(schema)
    try:
        hs = [t.pin_segment(s) for s in segs]
        for exact in (False, True):
            q = parse_query("SELECT SUM(md), AVG(md), COUNT(*) FROM t WHERE f < 60 GROUP BY d", exact_fp_sum=exact)
            o = oracle.run_groupby(schema, segs, q)
            with t.plan_execute(hs, q) as p:
                r = p.finalize()
                assert p.fp_sum_format(0)["mode"] == ("exact" if exact else "none")
            assert_same(r, o, q, schema)  # 1e-9 relative on the double sums
            assert r.stats.as_tuple() == o.stats
    finally:
        t.close()


def test_the_option_changes_nothing_for_integer_sums(data):
    """A query without a FLOAT / DOUBLE sum plans and answers exactly as without the option: same path, scan instance,
    table layout, values and statistics -- the partitioned pipeline included."""
    d = data(8193)
    for sql in ("SELECT SUM(f), COUNT(*), MIN(f), MAX(f), SUM(a1) FROM t GROUP BY a1, a2",
                "SELECT SUM(f), MAX(h1) FROM t WHERE f < 300 GROUP BY d", "SELECT SUM(f), AVG(a1) FROM t"):
        out = []
        for exact in (False, True):
            q = parse_query(sql, num_groups_limit=10 ** 9, exact_fp_sum=exact)
            with d.t.plan_execute(d.hs, q) as p:
                r = p.finalize()
                fm = [p.fp_sum_format(a) for a in range(len(q.aggregations))]
                assert all(f["mode"] == "none" for f in fm), fm
                geo = p.scan_geometry()
                out.append((p.group_path(), p.layout(), geo["variant"], geo["grid"], geo["lds_bytes"], r.as_dict(),
                            r.stats.as_tuple()))
        assert out[0] == out[1], sql
    assert out  # (the first query is the one the partitioned pipeline takes)
