"""The doc loop that the expression filter leaves (WHERE a * b > t) and the derived columns of group-by expressions
(GROUP BY a + b) share, at the doc counts where it decides something: one doc, one either side of a 64-doc wave step, of
the 256 docs a wave has in flight, of a wave's 2048-doc share and of a workgroup's 8192 docs.  One table, one segment per
count; planned and run segment by segment.  The yardstick is numpy over the columns: a and b are small INTs, so every
product and sum is an exact integer and every comparison below is integer equality -- no tolerance anywhere.  a has 24
distinct values (5 bits) and b 36 (6 bits: neither width divides a 32-bit word) in the segments that hold them all; the
short segments have the narrower widths of what they hold.

A leaf's bitmap is compared word for word, the zero bits from numDocs to the end of the last 64-bit word included.  The
last two docs of every segment are set, not drawn: the last one has the largest product and the one before it the
product 0, so the segment's last 64-doc step holds a match and a miss of every predicate below wherever it holds two
docs, and where it holds one (1, 65, 257, 2049, 8193 docs) that doc is the match of `>` and IN and the miss of NOT, with
the opposite answer right before it in the full step in front."""
import numpy as np
import pytest

from pinot_amd import _lib as L
from pinot_amd.executor import GpuTable
from pinot_amd.query import parse_query

pytestmark = pytest.mark.gpu

SCHEMA = [("g", "INT"), ("a", "INT"), ("b", "INT")]
DOCS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193)
A_LO, A_HI, B_LO, B_HI = -5, 18, 1, 36  # inclusive: 24 and 36 distinct values
T = 100                                  # a * b > T: about a third of the docs
IN_KEYS = (A_HI * B_HI, 36, 100, -60, 7)  # the largest product and four in the middle; never 0
K = 4                                    # CASE WHEN a < K
DTYPE = {L.INT: ">i4", L.LONG: ">i8", L.FLOAT: ">f4", L.DOUBLE: ">f8"}


def _columns(rng, n):
    c = {"g": rng.integers(0, 5, n), "a": rng.integers(A_LO, A_HI + 1, n), "b": rng.integers(B_LO, B_HI + 1, n)}
    c["a"][-1], c["b"][-1] = A_HI, B_HI  # the largest product: matches `> T` and the IN list
    if n > 1:
        c["a"][-2], c["b"][-2] = 0, B_LO  # the product 0: matches neither
    return c


@pytest.fixture(scope="module")
def data(oracle, gpu_lib):
    rng = np.random.default_rng(61)
    cols = [_columns(rng, n) for n in DOCS]
    t = GpuTable(SCHEMA)
    hs = [t.pin_segment(oracle.make_segment(SCHEMA, c)) for c in cols]
    yield t, hs, cols
    t.close()


def _q(sql):
    return parse_query(sql, filter_expressions=True, group_by_expressions=True)


# ------------------------------------------------------------------------------------------------ expression leaves
LEAVES = [("a * b > %d" % T, lambda p: p > T),
          ("a * b IN (%s)" % ", ".join(str(k) for k in IN_KEYS), lambda p: np.isin(p, IN_KEYS)),
          ("NOT (a * b > %d)" % T, lambda p: ~(p > T))]


@pytest.mark.parametrize("where,mask_of", LEAVES, ids=["gt", "in", "not_gt"])
def test_leaf_bitmap_is_the_mask_bit_for_bit(data, where, mask_of):
    t, hs, cols = data
    q = _q("SELECT COUNT(*) FROM t WHERE %s GROUP BY g" % where)
    for h, c in zip(hs, cols):
        n = len(c["a"])
        mask = mask_of(c["a"].astype(np.int64) * c["b"].astype(np.int64))
        # the yardstick first: the last 64-doc step decides both ways (see the module's docstring)
        last = mask[(n - 1) // 64 * 64:]
        if len(last) > 1:
            assert last.any() and not last.all(), (where, n)
        elif n > 1:
            assert last[0] != mask[n - 2], (where, n)
        words = (n + 63) // 64
        padded = np.zeros(words * 64, dtype=np.uint8)
        padded[:n] = mask
        want = np.packbits(padded, bitorder="little").view(np.uint64)
        got = t.filter_bitmap(h, q, n)
        assert got.dtype == np.uint64 and len(got) == words
        assert np.array_equal(got, want), (where, n)  # every word whole: the bits from n to the word's end are 0


# ------------------------------------------------------------------------------------------------ derived columns
DERIVED = [("a + b", lambda c: c["a"].astype(np.int64) + c["b"]),
           ("CASE WHEN a < %d THEN 0 ELSE 1 END" % K, lambda c: (c["a"] >= K).astype(np.int64))]


@pytest.mark.parametrize("expr,values_of", DERIVED, ids=["add", "case"])
def test_derived_column_dictionary_ids_and_counts(data, expr, values_of):
    t, hs, cols = data
    q = _q("SELECT COUNT(*) FROM t GROUP BY %s" % expr)
    gname = q.group_by[0]
    column = ("group", gname)
    seen = set()
    for h, c in zip(hs, cols):
        n = len(c["a"])
        vals = values_of(c)
        present, index, counts = np.unique(vals, return_inverse=True, return_counts=True)
        r = t.execute_groupby([h], q)
        # COUNT(*) per group
        assert r.as_dict() == {(int(v),): [int(k)] for v, k in zip(present, counts)}, (expr, n)
        # the dictionary the result's keys index: the table's, which holds the segments planned so far
        seen |= set(present.tolist())
        assert [int(v) for v in t.result_dictionary(r._holder.r, 0, gname, group_expr=True)] == sorted(seen), (expr, n)
        # the segment's own dictionary is the sorted set of the values present ...
        card, bits, dict_bytes, _ = t.segment_column_bytes(h, column)
        dvals = np.frombuffer(dict_bytes, dtype=DTYPE[t.group_types[gname]])
        assert card == len(present) and bits == max(1, int(card - 1).bit_length())
        assert np.array_equal(dvals.astype(np.int64), present) and np.array_equal(dvals, present), (expr, n)
        # ... and every doc's dictId is its value's index in it
        assert np.array_equal(t.read_dict_ids(h, column, np.arange(n)), index), (expr, n)
    assert [int(v) for v in t.dictionary(column)] == sorted(seen)
