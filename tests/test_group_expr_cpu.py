"""Expressions in GROUP BY, the parts that need no GPU: the parser's group_by_expressions flag (spellings, canonical
names, SELECT / ORDER BY binding, operands, result types, the default call and the limits as they were) and the host
steps of a derived column's build (pinot_amd/csrc/group_expr.h) run as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/group_expr_check.cpp), against numpy."""
import struct
import subprocess

import numpy as np
import pytest

import case_common as C
import expr_common as E
from pinot_amd import _lib as L
from pinot_amd import build
from pinot_amd.query import QueryContext, expr_type, parse_query

TYPES = {"i": "INT", "j": "INT", "l": "LONG", "fl": "FLOAT", "d": "DOUBLE", "s": "STRING", "a b": "INT"}
BUCKETS = "CASE WHEN i < 18 THEN 0 WHEN i < 65 THEN 1 ELSE 2 END"
BUCKETS_NAME = "case(less_than(i,18),less_than(i,65),0,1,2)"


def _q(sql):
    return parse_query(sql, group_by_expressions=True)


# ------------------------------------------------------------------------------------------------ parser
@pytest.mark.parametrize("item, name", [
    ("i * j", "mult(i,j)"),
    ("i + j * 2", "add(i,mult(j,2.0))"),
    ("(i + j) / d", "div(add(i,j),d)"),
    ("add(i, j)", "add(i,j)"),
    ("PLUS(i, j, l)", "add(i,j,l)"),
    ("div(d, sub(i, 1))", "div(d,sub(i,1.0))"),
    (BUCKETS, BUCKETS_NAME),
    ("case(greater_than(i, 1), 1, 0)", "case(greater_than(i,1),1,0)"),
    ('"a b" - 1', "sub(a b,1.0)"),
    ("CASE WHEN d > 0.5 THEN fl ELSE 0.1 END", "case(greater_than(d,0.5),fl,0.1)"),
])
def test_group_by_item_is_kept_as_its_function_form(item, name):
    q = _q("SELECT COUNT(*) FROM t GROUP BY %s" % item)
    assert q.group_by == [name]
    assert name in q.expressions and q.group_expr(name) == q.expressions[name]
    assert q.select == [("agg", "COUNT", "*")]


def test_plain_columns_stay_columns_under_the_flag():
    q = _q('SELECT g, "a b", SUM(i * j) FROM t GROUP BY g, "a b"')
    assert q.group_by == ["g", "a b"]
    assert set(q.expressions) == {"mult(i,j)"}  # the aggregation's argument alone
    assert q.group_expr("g") is None and q.group_expr("mult(i,j)") is None
    assert q.select[:2] == [("col", "g"), ("col", "a b")]


def test_select_and_order_by_bind_to_the_group_by_entry_in_any_spelling():
    q = _q("SELECT i * j, add(i, j), COUNT(*), SUM(i * j) FROM t WHERE i > 3 "
           "GROUP BY mult(i, j), i + j ORDER BY i*j DESC, plus(i,j), COUNT(*) LIMIT 5")
    assert q.group_by == ["mult(i,j)", "add(i,j)"]
    assert q.select == [("col", "mult(i,j)"), ("col", "add(i,j)"), ("agg", "COUNT", "*"), ("agg", "SUM", "mult(i,j)")]
    assert q.order_by == [(("col", "mult(i,j)"), False), (("col", "add(i,j)"), True), (("agg", "COUNT", "*"), True)]
    assert q.limit == 5
    assert q.expr_ref(("col", "add(i,j)")) == (L.ORDER_GROUP_BY, 1)
    assert q.expr_ref(("agg", "SUM", "mult(i,j)")) == (L.ORDER_AGGREGATION, 1)
    q = _q("SELECT %s, COUNT(*) FROM t GROUP BY %s ORDER BY %s" % (BUCKETS, BUCKETS, BUCKETS))
    assert q.select[0] == ("col", BUCKETS_NAME) and q.order_by == [(("col", BUCKETS_NAME), True)]


def test_an_expression_outside_group_by_is_refused():
    with pytest.raises(ValueError, match="no GROUP BY expression"):
        _q("SELECT i * j, COUNT(*) FROM t GROUP BY i + j")
    with pytest.raises(ValueError, match="no GROUP BY expression"):
        _q("SELECT COUNT(*) FROM t GROUP BY i ORDER BY i * 2")


def test_columns_lists_the_operands():
    q = _q("SELECT COUNT(*), SUM(d) FROM t WHERE fl > 1 GROUP BY g, i * j, CASE WHEN l > 3 THEN i ELSE 0 END")
    assert q.columns() == ["fl", "g", "i", "j", "l", "d"]


@pytest.mark.parametrize("item, rtype", [
    (BUCKETS, "INT"),
    ("CASE WHEN i > 0 THEN i ELSE j END", "INT"),
    ("CASE WHEN i > 0 THEN l ELSE 0 END", "LONG"),
    ("CASE WHEN i > 0 THEN 3000000000 ELSE 0 END", "LONG"),
    ("CASE WHEN d > 0.5 THEN 0.1 ELSE 0.0 END", "FLOAT"),
    ("CASE WHEN d > 0.5 THEN fl ELSE 0.5 END", "FLOAT"),
    ("CASE WHEN d > 0.5 THEN fl ELSE 1 END", "DOUBLE"),
    ("CASE WHEN i > 0 THEN d ELSE 0.1 END", "DOUBLE"),
    ("i * j", "DOUBLE"),
    ("i + 1", "DOUBLE"),
    ("CASE WHEN i > 0 THEN i ELSE 0 END * 2", "DOUBLE"),
])
def test_result_type(item, rtype):
    q = _q("SELECT COUNT(*) FROM t GROUP BY %s" % item)
    tree = q.expressions[q.group_by[0]]
    assert expr_type(tree, TYPES) == rtype
    cols = C.typed({"i": [1], "j": [1], "l": [1], "fl": [1.0], "d": [1.0]}, list(TYPES.items()))
    assert C.node_type(tree, cols) == rtype  # the yardstick's typing, which never calls expr_type


def test_string_operand_has_no_result_type():
    # (a STRING inside arithmetic is refused where the expression is registered: the C ABI names the column)
    q = _q("SELECT COUNT(*) FROM t GROUP BY CASE WHEN i > 0 THEN s ELSE 0 END")
    with pytest.raises(ValueError, match="STRING"):
        expr_type(q.expressions[q.group_by[0]], TYPES)


@pytest.mark.parametrize("sql", [
    "SELECT COUNT(*) FROM t GROUP BY i * j",
    "SELECT COUNT(*) FROM t GROUP BY add(i, j)",
    "SELECT COUNT(*) FROM t GROUP BY g, i + 1",
    "SELECT COUNT(*) FROM t GROUP BY %s" % BUCKETS,
])
def test_the_default_call_still_raises(sql):
    with pytest.raises(ValueError, match="expressions are supported inside aggregations only"):
        parse_query(sql)


def test_query_context_reads_an_expression_from_its_dict_and_never_sniffs():
    with pytest.raises(ValueError, match="expressions are supported inside aggregations only"):
        QueryContext(["i+j"], [("COUNT", "*")])
    tree = _q("SELECT COUNT(*) FROM t GROUP BY i + j").expressions["add(i,j)"]
    q = QueryContext(["g", "add(i,j)"], [("COUNT", "*"), ("SUM", "add(i,j)")], expressions={"add(i,j)": tree})
    assert q.group_expr("add(i,j)") == tree and q.group_expr("g") is None
    assert q.columns() == ["g", "i", "j"]
    # the C form names the derived column's index, not the aggregation's virtual column of the same name
    index = {"g": 0, "i": 1, "j": 2, "add(i,j)": 3, ("group", "add(i,j)"): L.GROUP_EXPR_COLUMN_BASE + 5}
    c, keep = q.to_c(index)
    assert [c.group_by[k] for k in range(c.num_group_by)] == [0, L.GROUP_EXPR_COLUMN_BASE + 5]
    assert c.aggs[1].column == 3
    with pytest.raises(KeyError):
        q2 = QueryContext(["add(i,j)"], [("COUNT", "*")], expressions={"add(i,j)": tree})
        q2.to_c({"i": 1, "j": 2, "add(i,j)": 3})  # no derived column registered


def test_the_limits_and_their_messages_are_an_aggregation_arguments():
    long_sum = " + ".join("i" for _ in range(9))
    for make in (lambda e: "SELECT SUM(%s) FROM t" % e, lambda e: "SELECT COUNT(*) FROM t GROUP BY %s" % e):
        with pytest.raises(ValueError, match=r"needs an evaluation stack of \d+, more than 4|compiles to \d+ ops, more than 16"):
            _q(make(long_sum))
        with pytest.raises(ValueError, match="names 5 columns, more than 4"):
            _q(make("ADD(a, b, c, d, e)"))
        with pytest.raises(ValueError, match="literal-only expression"):
            _q(make("1 + 2"))
        with pytest.raises(ValueError, match="CASE without ELSE"):
            _q(make("CASE WHEN i > 1 THEN 2 END"))
        with pytest.raises(ValueError, match="used as a number"):
            _q(make("greater_than(i, 1)"))
    # the messages are the same text in both places
    msgs = []
    for sql in ("SELECT SUM(ADD(a, b, c, d, e)) FROM t", "SELECT COUNT(*) FROM t GROUP BY ADD(a, b, c, d, e)"):
        with pytest.raises(ValueError) as ei:
            _q(sql)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]


# ------------------------------------------------------------------------------------------------ host steps
NAN2 = struct.unpack("<d", struct.pack("<Q", 0xfff8000000000001))[0]  # a NaN that is not the canonical one
DTYPE = {0: ">i4", 1: ">i8", 2: ">f4", 3: ">f8"}


def _hex(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _run_check(cases):
    """cases: [(type code, candidate doubles, doc doubles)] -> per case (card, bits, width, ncand, dict bytes, remap, ids)."""
    lines = []
    for ty, cand, docs in cases:
        lines.append("build %d %d %d" % (ty, len(cand), len(docs)))
        lines.append(" ".join(_hex(v) for v in cand))
        lines.append(" ".join(_hex(v) for v in docs))
    res = subprocess.run([build.build_group_expr_check()], input="\n".join(lines) + "\n", stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout.strip().split("\n")
    assert len(out) == 4 * len(cases)
    got = []
    for k in range(len(cases)):
        head = out[4 * k].split()
        got.append((int(head[1]), int(head[3]), int(head[5]), int(head[7]), bytes.fromhex(out[4 * k + 1][5:]),
                    [int(x) for x in out[4 * k + 2].split()[1:]], [int(x) for x in out[4 * k + 3].split()[1:]]))
    return got


def _expect(ty, cand, docs):
    """numpy's answer: keys in the dictionaries' order, the docs' distinct keys as the dictionary, typed bytes."""
    ckeys = np.unique(C.keys(np.asarray(cand, dtype=np.float64)))
    dkeys = C.keys(np.asarray(docs, dtype=np.float64)) if len(docs) else np.zeros(0, dtype=np.int64)
    present = np.unique(dkeys)
    remap = [int(np.searchsorted(present, k)) if k in set(present.tolist()) else -1 for k in ckeys.tolist()]
    ids = np.searchsorted(present, dkeys).tolist()
    vals = np.array([E.from_bits(E.NAN_KEY) if k == E.NAN_KEY else
                     E.from_bits((k if k >= 0 else k ^ (2 ** 63 - 1)) & (2 ** 64 - 1)) for k in present.tolist()],
                    dtype=np.float64)
    dict_bytes = vals.astype(np.int64).astype(DTYPE[ty]).tobytes() if ty < 2 else vals.astype(DTYPE[ty]).tobytes()
    card = len(present)
    bits = 1 if card <= 2 else int(card - 1).bit_length()
    return card, bits, 4 if ty in (0, 2) else 8, len(ckeys), dict_bytes, remap, ids


def test_host_steps_cardinalities_and_bits():
    rng = np.random.default_rng(5)
    cases = []
    for card in (1, 2, 3, 4, 5, 8, 9, 256, 257, 4096, 4097):
        vals = (np.arange(card) * 3 - 7).astype(np.float64)
        cand = rng.permutation(np.concatenate([vals, vals[: card // 2], [1e9, -1e9, 0.5]]))  # duplicates and unused ones
        docs = rng.permutation(np.concatenate([vals, rng.choice(vals, 50)]))
        for ty in (0, 1, 3):
            cases.append((ty, cand.tolist(), docs.tolist()))
    got = _run_check(cases)
    for (ty, cand, docs), g in zip(cases, got):
        want = _expect(ty, cand, docs)
        assert g == want, (ty, len(set(docs)), g[:4], want[:4])
        assert g[5].count(-1) == 3  # the unused candidates have no dictId


def test_host_steps_special_values_and_types():
    special = [0.0, -0.0, float("nan"), NAN2, float("inf"), float("-inf"), 1.5, -1.5, 5e-324, -5e-324]
    f32 = [float(np.float32(x)) for x in (0.1, -0.1, 2.5, 3.4e38)] + [0.0, -0.0, float("nan"), float("inf")]
    cases = [(3, special + [7.0], special + special[:4]),      # DOUBLE: -0.0 and +0.0 apart, the NaNs one value, on top
             (2, f32 + [1.0], f32 + f32),                      # FLOAT: the doubles are (double)(float) of one
             (1, [2.0 ** 53, -2.0 ** 53, 0.0, 3.0], [2.0 ** 53, -2.0 ** 53, 3.0]),  # LONG at the exact range's ends
             (0, [2147483647.0, -2147483648.0, 0.0], [2147483647.0, -2147483648.0, 0.0, 0.0]),
             (3, [1.0, 2.0], []),                              # no docs: an empty dictionary, every candidate unused
             (0, [], [])]
    got = _run_check(cases)
    for (ty, cand, docs), g in zip(cases, got):
        assert g == _expect(ty, cand, docs), (ty, g, _expect(ty, cand, docs))
    card, bits, width, ncand, dbytes, remap, ids = got[0]
    vals = np.frombuffer(dbytes, dtype=">f8")
    assert card == 9 and ncand == 10  # the two NaNs are one candidate and one value
    assert np.signbit(vals[3]) and vals[3] == 0 and not np.signbit(vals[4]) and vals[4] == 0  # -0.0 right below +0.0
    assert np.isnan(vals[-1]) and np.isinf(vals[-2])  # NaN above +inf
    assert dbytes[-8:] == bytes.fromhex("7ff8000000000000")
    assert got[4][0] == 0 and got[4][1] == 1 and got[4][5] == [-1, -1]
    assert got[5][:4] == (0, 1, 4, 0)
