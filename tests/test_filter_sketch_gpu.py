"""Byte-code sketches of wide filter columns on the GPU (col_sketch.h, rt_sketch.cpp, k_sketch.hip).

Every case runs on two tables holding the same segments, one with sketches (the default) and one without
(set_filter_sketch(0) before the pins).  Both must equal the oracle in groups, values and the full statistics tuple, and
each other; Plan.sketch_leaves() must say which (scanned segment, scan leaf) pairs read the 8-bit codes.

Segments have 70 005 docs: nine 8192-doc tiles, a partial last 32-doc group.  Column `a` holds 5 000 distinct values (13
bits) with Zipf-like doc counts, its hot values scattered over the dictionary; `b` has 400 values (9 bits: never
sketched); k1, k2 (2 000 values each, 11 bits) make a 4 M-key space for the partitioned group-by.  The sketch a segment
got is read back through segment_sketch_info and recomputed here from the value arrays before any case relies on it.
"""
import numpy as np
import pytest

from pinot_amd.executor import GpuTable
from pinot_amd.query import parse_query

pytestmark = pytest.mark.gpu

DOCS = 70005
CARD_A = 5000
SCHEMA = [("a", "INT"), ("b", "INT"), ("g", "INT"), ("k1", "INT"), ("k2", "INT"), ("m1", "INT"), ("m2", "LONG"),
          ("x", "DOUBLE")]
HOT = 127
TILE_DOCS = 8192


def val_a(dict_id):
    """Column a's value of dictId `dict_id` (every value occurs in every segment); 1001 is in no dictionary."""
    return 1000 + 7 * int(dict_id)


def zipf_ids(n, card, step, offset, rng):
    """n dictIds in [0, card), every id at least once, doc counts ~ 1 / (rank + 1), the id of rank r at (r * step +
    offset) mod card (step coprime with card): the hot ids lie `step` apart, with cold ids between them."""
    ranks = np.arange(card)
    lo, hi = 0, n
    while lo < hi:  # the largest C whose counts fit
        c = (lo + hi + 1) // 2
        if int((c // (ranks + 1) + 1).sum()) <= n:
            lo = c
        else:
            hi = c - 1
    counts = lo // (ranks + 1) + 1
    counts[0] += n - int(counts.sum())
    ids = np.repeat((ranks * step + offset) % card, counts)
    assert len(ids) == n and len(np.unique(ids)) == card
    return rng.permutation(ids)


def padded_sketch_bytes(n):
    return (((n + TILE_DOCS - 1) // TILE_DOCS) * 256 * 8 + 4) * 4


def expected_sketch(ids, card):
    """(first_id, singleton docs) of the sketch of a column with these dictIds, recomputed: the 127 ids of the largest
    counts (ties to the lower id) are codes of their own, the ids between them interval codes."""
    counts = np.bincount(ids, minlength=card)
    order = sorted((i for i in range(card) if counts[i] > 0), key=lambda i: (-counts[i], i))[:HOT]
    bounds = {0}
    for h in order:
        bounds.add(h)
        if h + 1 < card:
            bounds.add(h + 1)
    return sorted(bounds) + [card], int(counts[order].sum()), order


def main_columns(seed, offset):
    rng = np.random.default_rng(seed)
    i = np.arange(DOCS)
    k1, k2 = rng.integers(0, 2000, DOCS), rng.integers(0, 2000, DOCS)
    k1[:2000] = np.arange(2000)
    k2[:2000] = np.arange(2000)
    b = rng.integers(0, 400, DOCS)
    b[:400] = np.arange(400)
    ids = zipf_ids(DOCS, CARD_A, 37, offset, rng)
    return {"a": 1000 + 7 * ids, "b": b, "g": i % 7, "k1": k1, "k2": k2, "m1": rng.integers(-50, 50, DOCS),
            "m2": rng.integers(0, 10 ** 6, DOCS), "x": (i % 64 - 20) * 0.25}, ids


class Pair:
    """The same segments on a table with sketches and on one without."""

    def __init__(self, oracle, schema, columns):
        self.oracle, self.schema = oracle, schema
        self.on, self.off = GpuTable(schema), GpuTable(schema)
        self.off.set_filter_sketch(0)
        self.empty_bytes = (self.on.device_bytes(), self.off.device_bytes())
        self.segs = [oracle.make_segment(schema, c) for c in columns]
        self.h_on = [self.on.pin_segment(s) for s in self.segs]
        self.h_off = [self.off.pin_segment(s) for s in self.segs]
        self.pinned_bytes = (self.on.device_bytes(), self.off.device_bytes())

    def close(self):
        self.on.close()
        self.off.close()

    def run(self, q, which=None, config=None, path=None, variants=None, use_oracle=True):
        """The query on both tables over the segments `which` (all); returns (result with sketches, its
        sketch_leaves()).  Asserts the two tables agree with the oracle (use_oracle=False: an aggregation the oracle
        does not have) and with each other."""
        which = list(range(len(self.segs))) if which is None else which
        exp = self.oracle.run_groupby(self.schema, [self.segs[i] for i in which], q) if use_oracle else None
        out = []
        for t, hs in ((self.on, self.h_on), (self.off, self.h_off)):
            if config:
                t.set_config(**config)
            try:
                with t.plan([hs[i] for i in which], q) as p:
                    leaves = p.sketch_leaves()
                    p.execute()
                    r = p.finalize()
                    if path is not None:
                        assert p.group_path() == path, p.group_path()
                    if variants is not None:
                        assert int(p.scan_geometry()["variant"]) in variants, p.scan_geometry()
            finally:
                if config:
                    t.reset_config()
            if exp is not None:
                assert r.as_dict() == exp.groups
                assert r.stats.as_tuple() == tuple(exp.stats)
            out.append((r, leaves))
        (r_on, l_on), (r_off, l_off) = out
        assert r_on.as_dict() == r_off.as_dict() and r_on.stats.as_tuple() == r_off.stats.as_tuple()
        assert l_off == (0, 0), "a table with sketches off plans none"
        return r_on, l_on


@pytest.fixture(scope="module")
def main(oracle, gpu_lib):
    c1, ids1 = main_columns(7, 0)
    c2, ids2 = main_columns(8, 18)  # the hot ids of segment 1 lie between the hot ids of segment 2
    pair = Pair(oracle, SCHEMA, [c1, c2])
    info = [pair.on.segment_sketch_info(h, "a") for h in pair.h_on]
    yield pair, (ids1, ids2), info
    pair.close()


def _q(where, group_by="g", **kw):
    return parse_query("SELECT COUNT(*), SUM(m1), SUM(m2) FROM t WHERE %s GROUP BY %s" % (where, group_by), **kw)


def _code_of(first_id, dict_id):
    return int(np.searchsorted(first_id, dict_id, side="right")) - 1


def _cold_sharing_a_code(first_id, hot):
    """A dictId that is not hot and whose code holds at least two dictIds."""
    hot = set(hot)
    for c in range(len(first_id) - 1):
        if first_id[c + 1] - first_id[c] >= 2:
            assert first_id[c] not in hot and first_id[c] + 1 not in hot
            return int(first_id[c]) + 1
    raise AssertionError("no interval code of two dictIds")


def test_the_sketch_the_segments_got(main):
    """Column a of both segments has a sketch: at most 256 codes, the recomputed boundaries, singleton codes covering
    well over 1/8 of the docs; the 9- and 11-bit columns have none; with sketches off nothing has one."""
    pair, ids, info = main
    for k in range(2):
        first_id, docs, _ = expected_sketch(ids[k], CARD_A)
        assert info[k] is not None
        assert info[k]["ncodes"] == len(first_id) - 1 <= 256
        assert info[k]["first_id"].tolist() == first_id
        assert info[k]["singleton_docs"] == docs and docs > DOCS // 2
        assert info[k]["bytes"] == padded_sketch_bytes(DOCS)
        for name in ("b", "g", "k1", "k2", "m1"):
            assert pair.on.segment_sketch_info(pair.h_on[k], name) is None, name
        # m2: 20 bits and uniform -- the sketch is discarded (cover far below 1/8)
        assert pair.on.segment_sketch_info(pair.h_on[k], "m2") is None
        for name, _ in SCHEMA:
            assert pair.off.segment_sketch_info(pair.h_off[k], name) is None, name


def test_device_bytes(main):
    """The table's device bytes grow by exactly the padded code bytes of every kept sketch."""
    pair, _, info = main
    on, off = pair.pinned_bytes
    assert on - off == 2 * padded_sketch_bytes(DOCS) == sum(i["bytes"] for i in info)


def _cases(ids1, info1):
    first_id, _, hot = expected_sketch(ids1, CARD_A)
    h1, h2 = hot[0], hot[1]
    assert abs(h1 - h2) > 1, "two hot ids that are not neighbours: an IN of them is a set, not a range"
    cold = _cold_sharing_a_code(first_id, hot)
    # a range of three whole codes that starts with an interval code of at least two dictIds
    c = next(c for c in range(len(first_id) - 4) if first_id[c + 1] - first_id[c] >= 2)
    lo, hi = first_id[c], first_id[c + 3]
    return {
        "c3 shape": ("b BETWEEN 100 AND 180 AND a = %d" % val_a(h1), (1, 0)),
        "cold": ("a = %d" % val_a(cold), (0, 1)),
        "not equal hot": ("a <> %d" % val_a(h1), (1, 0)),
        "in hot hot": ("a IN (%d, %d)" % (val_a(h1), val_a(h2)), (1, 0)),
        "in hot cold": ("a IN (%d, %d)" % (val_a(h1), val_a(cold)), (0, 1)),
        "not in hot hot": ("a NOT IN (%d, %d)" % (val_a(h1), val_a(h2)), (1, 0)),
        "range on code boundaries": ("a BETWEEN %d AND %d" % (val_a(lo), val_a(hi - 1)), (1, 0)),
        "range moved by one dictId": ("a BETWEEN %d AND %d" % (val_a(lo + 1), val_a(hi - 1)), (0, 1)),
        "range end moved by one dictId": ("a BETWEEN %d AND %d" % (val_a(lo), val_a(hi)), None),
        "or": ("a = %d OR b = 5" % val_a(h1), (1, 0)),
        "not": ("NOT (a = %d OR b = 5)" % val_a(h1), (1, 0)),
        "or with a cold leaf": ("a = %d OR a = %d OR b = 5" % (val_a(h1), val_a(cold)), (0, 2)),
        "hot and not cold": ("a = %d AND a <> %d" % (val_a(h1), val_a(cold)), (0, 2)),
    }


CASE_NAMES = ["c3 shape", "cold", "not equal hot", "in hot hot", "in hot cold", "not in hot hot",
              "range on code boundaries", "range moved by one dictId", "range end moved by one dictId", "or", "not",
              "or with a cold leaf", "hot and not cold"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case(main, name):
    pair, ids, info = main
    where, want = _cases(ids[0], info[0])[name]
    if want is None:  # the end one dictId further: exact only if that dictId is a code of its own
        first_id, _, _ = expected_sketch(ids[0], CARD_A)
        hi = int(where.rsplit(" ", 1)[1])
        hi_id = (hi - 1000) // 7 + 1
        want = (1, 0) if hi_id in first_id else (0, 1)
    r, leaves = pair.run(_q(where), which=[0])
    assert leaves == want
    assert r.stats.num_docs_scanned > 0


def test_absent_value_folds_as_before(main):
    pair, _, _ = main
    r, leaves = pair.run(_q("a = 1001"), which=[0])
    assert leaves == (0, 0) and r.as_dict() == {}


def test_dense_instance(main):
    pair, ids, _ = main
    hot = expected_sketch(ids[0], CARD_A)[2]
    _, leaves = pair.run(_q("a = %d" % val_a(hot[0])), which=[0], config={"dense_selectivity": 0.0}, variants=(1, 2))
    assert leaves == (1, 0)
    first_id = expected_sketch(ids[0], CARD_A)[0]
    cold = _cold_sharing_a_code(first_id, hot)
    _, leaves = pair.run(_q("a <> %d" % val_a(cold)), which=[0], config={"dense_selectivity": 0.0}, variants=(1, 2))
    assert leaves == (0, 1)


# (variant numbers: internal.h ScanVariant)
FAMILIES = [("fx", "SUM(x), COUNT(*)", {"exact_fp_sum": True}, (6, 7), True),
            ("dc", "DISTINCTCOUNT(b), COUNT(*)", {}, (8, 9), False),
            ("hist", "PERCENTILE(m1, 50), COUNT(*)", {}, (10, 11), False),
            ("expr", "SUM(m1 * m2), COUNT(*)", {}, (12, 13), False)]


@pytest.mark.parametrize("name,select,kw,variants,use_oracle", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_scan_families(main, name, select, kw, variants, use_oracle):
    """The FX, DC, HIST and EXPR instances share the scan's body: each reads the sketch for the hot-id filter and gives
    what the table without sketches gives (and the oracle, where it has the aggregation); the counts are the value
    arrays'."""
    pair, ids, _ = main
    first_id, _, hot = expected_sketch(ids[0], CARD_A)
    for dict_id, want in ((hot[0], (1, 0)), (_cold_sharing_a_code(first_id, hot), (0, 1))):
        q = parse_query("SELECT %s FROM t WHERE a = %d GROUP BY g" % (select, val_a(dict_id)), **kw)
        r, leaves = pair.run(q, which=[0], variants=variants, use_oracle=use_oracle)
        assert leaves == want
        got = r.as_dict()
        g = (np.arange(DOCS) % 7)[ids[0] == dict_id]
        assert {k[0]: row[1] for k, row in got.items()} == {int(k): int((g == k).sum()) for k in np.unique(g)}
        if name == "dc":
            b = main_columns(7, 0)[0]["b"][ids[0] == dict_id]
            assert {k[0]: row[0] for k, row in got.items()} == {int(k): len(np.unique(b[g == k])) for k in np.unique(g)}


def test_partitioned_path(main):
    pair, ids, _ = main
    first_id, _, hot = expected_sketch(ids[0], CARD_A)
    q = _q("a = %d" % val_a(hot[0]), group_by="k1, k2", num_groups_limit=10 ** 9)
    _, leaves = pair.run(q, which=[0], path="partitioned")
    assert leaves == (1, 0)
    q = _q("a = %d" % val_a(_cold_sharing_a_code(first_id, hot)), group_by="k1, k2", num_groups_limit=10 ** 9)
    _, leaves = pair.run(q, which=[0], path="partitioned")
    assert leaves == (0, 1)


def test_hot_in_one_segment_cold_in_the_other(main):
    """The swap is per segment: segment 1's hottest value shares a code in segment 2."""
    pair, ids, info = main
    h1 = expected_sketch(ids[0], CARD_A)[2][0]
    f2, _, hot2 = expected_sketch(ids[1], CARD_A)
    c = _code_of(f2, h1)
    assert h1 not in hot2 and f2[c + 1] - f2[c] >= 2
    _, leaves = pair.run(_q("a = %d" % val_a(h1)))
    assert leaves == (1, 1)
    _, leaves = pair.run(_q("b BETWEEN 100 AND 180 AND a = %d" % val_a(h1)))
    assert leaves == (1, 1)


def test_filter_bitmap(main):
    """K2: the filter's docId bitmap, with sketches on and off, against the value arrays."""
    pair, ids, _ = main
    hot = expected_sketch(ids[0], CARD_A)[2]
    q = _q("a = %d" % val_a(hot[0]))
    want = ids[0] == hot[0]
    words = [t.filter_bitmap(hs[0], q, DOCS) for t, hs in ((pair.on, pair.h_on), (pair.off, pair.h_off))]
    assert (words[0] == words[1]).all()
    got = np.unpackbits(words[0].view(np.uint8), bitorder="little")[:DOCS].astype(bool)
    assert 0 < want.sum() < DOCS and (got == want).all()


def test_switching_planning_off_and_on(main):
    """min_bits = 0 also stops plans from reading the sketches already pinned; the default brings them back."""
    pair, ids, _ = main
    q = _q("a = %d" % val_a(expected_sketch(ids[0], CARD_A)[2][0]))
    pair.on.set_filter_sketch(0)
    try:
        with pair.on.plan(pair.h_on[:1], q) as p:
            assert p.sketch_leaves() == (0, 0)
    finally:
        pair.on.set_filter_sketch()
    with pair.on.plan(pair.h_on[:1], q) as p:
        assert p.sketch_leaves() == (1, 0)


W_SCHEMA = [("c11", "INT"), ("c12", "INT"), ("u13", "INT"), ("v", "INT")]
W_DOCS = 20000


def test_widths_cover_rule_and_memory(oracle, gpu_lib):
    """A skewed column of 11 bits gets no sketch, one of 12 bits does; a uniform 13-bit column's sketch is discarded (its
    127 most frequent values hold a few per cent of the docs).  device_bytes grows by the one kept sketch and returns to
    the empty table's value after the unpins."""
    rng = np.random.default_rng(11)
    u = rng.integers(0, 5000, W_DOCS)
    u[:5000] = np.arange(5000)
    i11, i12 = zipf_ids(W_DOCS, 2000, 37, 0, rng), zipf_ids(W_DOCS, 4000, 37, 0, rng)
    cols = {"c11": i11 * 3, "c12": i12 * 3, "u13": u, "v": np.arange(W_DOCS) % 97}
    pair = Pair(oracle, W_SCHEMA, [cols])
    try:
        on, off = pair.on, pair.off
        h = pair.h_on[0]
        assert on.segment_column_bytes(h, "c11")[1] == 11 and on.segment_column_bytes(h, "c12")[1] == 12
        assert on.segment_column_bytes(h, "u13")[1] == 13
        assert on.segment_sketch_info(h, "c11") is None
        assert on.segment_sketch_info(h, "u13") is None
        info = on.segment_sketch_info(h, "c12")
        first_id, docs, hot = expected_sketch(i12, 4000)
        assert info is not None and info["first_id"].tolist() == first_id and info["singleton_docs"] == docs
        assert docs * 8 >= W_DOCS
        assert pair.pinned_bytes[0] - pair.pinned_bytes[1] == padded_sketch_bytes(W_DOCS) == info["bytes"]
        q = parse_query("SELECT COUNT(*), SUM(v) FROM t WHERE c12 = %d AND c11 = 0 AND u13 < 2500 GROUP BY v" % (3 * hot[0]))
        r, leaves = pair.run(q)
        assert leaves == (1, 0) and r.stats.num_docs_scanned > 0
        on.unpin_segment(h)
        off.unpin_segment(pair.h_off[0])
        assert (on.device_bytes(), off.device_bytes()) == pair.empty_bytes
    finally:
        pair.close()
