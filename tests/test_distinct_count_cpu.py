"""DISTINCTCOUNT without a GPU: the fixture of the reference's answers (InterSegmentAggregationSingleValueQueriesTest.
testDistinctCount, :176-195) reproduces from the KAT segment's columns by a numpy set count, and the query model, the
bindings and the header carry the function (code 5)."""
import os
import re

import numpy as np

import distinct_common as D
import kat_common as K
from pinot_amd import _lib as L
from pinot_amd.executor import aggregation_defaults
from pinot_amd.query import AGG_FUNCTIONS, QueryContext, parse_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_values_reproduce_from_the_segment():
    """The eight recorded values: 4 copies of the segment hold the same value sets as one."""
    cols = K.sv_columns()
    n = len(cols["column1"])
    assert n * 4 == D.KAT_DISTINCT["cases"][0]["stats"][3]
    seen = 0
    for case in D.KAT_DISTINCT["cases"]:
        mask = D.json_filter_mask(K.KAT["query_filter"] if case["filter"] else None, cols, n)
        assert int(mask.sum()) * 4 == case["stats"][0], case["variant"]
        gb = [cols[D.KAT_DISTINCT["group_by_column"]]] if case["group_by"] else []
        counts = D.distinct_counts(gb, [cols["column1"], cols["column3"]], mask)
        top = [max(v[a] for v in counts.values()) for a in range(2)]  # PQL: the top group per function
        assert [str(x) for x in top] == case["values"], (case["variant"], top)
        # docs x distinct group-by and aggregation columns; the dictionary-based plan scans nothing
        projected = 2 + (1 if case["group_by"] else 0)
        exempt = not case["group_by"] and not case["filter"]
        assert case["stats"][2] == (0 if exempt else case["stats"][0] * projected)
        seen += len(top)
    assert seen == 8


def _fns(q, index):
    c, keep = q.to_c(index)
    return [c.aggs[i].fn for i in range(c.num_aggs)], [c.aggs[i].column for i in range(c.num_aggs)]


def test_to_c_gives_code_5():
    index = {"g": 0, "x": 1}
    assert L.AGG_DISTINCTCOUNT == 5 and AGG_FUNCTIONS["DISTINCTCOUNT"] == 5
    for name in ("DISTINCTCOUNT", "DISTINCT_COUNT", "distinctCount", "distinct_count"):
        q = parse_query("SELECT COUNT(*), %s(x) FROM t GROUP BY g" % name)
        assert q.aggregations == [("COUNT", "*"), ("DISTINCTCOUNT", "x")]
        assert _fns(q, index) == ([0, 5], [-1, 1])


def test_query_context_normalises_the_name():
    q = QueryContext(["g"], [("distinct_count", "x"), ("SUM", "x")])
    assert q.aggregations[0] == ("DISTINCTCOUNT", "x")
    assert _fns(q, {"g": 0, "x": 1})[0] == [5, 1]


def test_order_by_reference_resolves():
    q = parse_query("SELECT g, DISTINCT_COUNT(x) FROM t GROUP BY g ORDER BY DISTINCTCOUNT(x) DESC LIMIT 3")
    assert q.aggregations == [("DISTINCTCOUNT", "x")]
    assert q.expr_ref(q.order_by[0][0]) == (L.ORDER_AGGREGATION, 0)


def test_default_over_no_documents_is_zero():
    d = aggregation_defaults([("DISTINCTCOUNT", "x"), ("COUNT", "*")])
    assert d == [0, 0] and isinstance(d[0], int)


def test_header_declares_the_enumerator():
    text = open(os.path.join(ROOT, "include", "pinotgpu.h")).read()
    m = re.search(r"enum pgpu_agg_fn \{([^}]*)\}", text)
    assert m and re.search(r"PGPU_AGG_DISTINCTCOUNT\s*=\s*5\b", m.group(1))
    assert re.search(r"#define PGPU_ABI_VERSION 3\b", text)
    assert np.int64(5) == L.AGG_DISTINCTCOUNT
