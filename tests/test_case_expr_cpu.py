"""Conditional expressions (CASE WHEN inside aggregations and WHERE) without a GPU: the grammar and the canonical
function form, the reference's literal typing and CASE result type, every declined shape, the limits, and the host
evaluator (tools/case_check.cpp over pinot_amd/csrc/expr_eval.h, under AddressSanitizer + UndefinedBehaviorSanitizer
with contraction off) against the typed numpy yardstick of case_common.py, bit for bit.

pgpu_table_add_expression itself needs a device to make its table; its verdicts on badly typed programs are
expr_compile's, which the tool prints here, and tests/test_case_expr_gpu.py asks the C ABI for them."""
import subprocess

import numpy as np
import pytest

import case_common as C
import expr_common as E
from pinot_amd import _lib as L
from pinot_amd import build
from pinot_amd import query as Q
from pinot_amd.query import QueryContext, expr_columns, expr_name, expr_program, parse_expression, parse_query

COL, LIT, SEL = L.EXPR_COLUMN, L.EXPR_LITERAL, L.EXPR_SELECT
TYPES = {"i": "INT", "j": "INT", "l": "LONG", "f": "FLOAT", "d": "DOUBLE", "e": "DOUBLE", "s": "STRING"}


def test_opcodes_follow_div():
    assert (L.EXPR_EQ, L.EXPR_NE, L.EXPR_GT, L.EXPR_GE, L.EXPR_LT, L.EXPR_LE, L.EXPR_AND, L.EXPR_OR, L.EXPR_SELECT) == \
        tuple(range(6, 15))


# ------------------------------------------------------------------------------------------------ parsing
def test_sql_and_function_form_are_one_tree():
    sql = parse_expression("CASE WHEN clicks > 100 THEN 1 WHEN clicks > 10 THEN 0.5 ELSE 0 END")
    fn = parse_expression("case(greater_than(clicks,100),greater_than(clicks,10),1,0.5,0)")
    # the reference's argument order: the whens, then the thens, then the else
    assert sql == fn == ("case", [("greater_than", [("col", "clicks"), ("lit", "100")]),
                                  ("greater_than", [("col", "clicks"), ("lit", "10")]),
                                  ("lit", "1"), ("lit", "0.5"), ("lit", "0")])
    assert expr_name(sql) == "case(greater_than(clicks,100),greater_than(clicks,10),1,0.5,0)"
    assert parse_expression(expr_name(sql)) == sql
    for op, name in (("=", "equals"), ("!=", "not_equals"), ("<>", "not_equals"), ("<", "less_than"),
                     ("<=", "less_than_or_equal"), (">", "greater_than"), (">=", "greater_than_or_equal")):
        assert expr_name(parse_expression("CASE WHEN a %s b THEN 1 ELSE 0 END" % op)) == "case(%s(a,b),1,0)" % name


def test_literals_keep_their_typed_text_where_the_type_counts():
    t = parse_expression("CASE WHEN a > 0 THEN 0 WHEN a > 0.0 THEN 1e10 WHEN a > -2.50 THEN 100.0 ELSE 12345678.5 END")
    assert expr_name(t) == "case(greater_than(a,0),greater_than(a,0.0),greater_than(a,-2.5),0,1.0E10,100.0,1.23456785E7)"
    # inside an arithmetic node a literal is named as before
    assert expr_name(parse_expression("CASE WHEN a * 2 > 1 THEN b * 2 ELSE 0 END")) == \
        "case(greater_than(mult(a,2.0),1),mult(b,2.0),0)"
    assert expr_name(parse_expression("a * 2")) == "mult(a,2.0)"
    for raw, text in (("0.001", "0.001"), ("0.0001", "1.0E-4"), ("9999999.5", "9999999.5"), ("10000000", "10000000"),
                      ("1e7", "1.0E7"), ("1e-3", "0.001"), ("-0.0", "-0.0"), ("007", "7"), ("1.50", "1.5"),
                      ("123456789012345", "123456789012345"), ("1e22", "1.0E22"), ("0.5e-9", "5.0E-10")):
        assert Q.typed_literal_text(raw) == text


def test_conditions_and_or_parentheses():
    t = parse_expression("CASE WHEN a > 1 AND (b < 2 OR c = 3) THEN x ELSE 0 END")
    assert expr_name(t) == "case(and(greater_than(a,1),or(less_than(b,2),equals(c,3))),x,0)"
    assert expr_name(parse_expression("CASE WHEN (a + b) / 2 > c THEN x ELSE 0 END")) == \
        "case(greater_than(div(add(a,b),2.0),c),x,0)"
    assert expr_name(parse_expression("CASE WHEN a > 1 OR b > 1 AND c > 1 THEN x ELSE 0 END")) == \
        "case(or(greater_than(a,1),and(greater_than(b,1),greater_than(c,1))),x,0)"
    assert expr_name(parse_expression("case(and(equals(a,1),not_equals(b,2)),x,y)")) == "case(and(equals(a,1),not_equals(b,2)),x,y)"
    assert expr_columns(t) == ["a", "b", "c", "x"]


def test_case_stands_where_a_factor_may():
    q = parse_query("SELECT g, SUM(CASE WHEN a > 1 THEN b ELSE 0 END / c), SUM(CASE WHEN a > 1 THEN b ELSE 0 END * c), "
                    "COUNT(CASE WHEN a > 1 THEN b ELSE 0 END) FROM t WHERE g < 3 GROUP BY g "
                    "ORDER BY SUM(CASE WHEN a > 1 THEN b ELSE 0 END / c) DESC LIMIT 3")
    assert q.aggregations == [("SUM", "div(case(greater_than(a,1),b,0),c)"), ("SUM", "mult(case(greater_than(a,1),b,0),c)"),
                              ("COUNT", "case(greater_than(a,1),b,0)")]
    assert q.order_by == [(("agg", "SUM", "div(case(greater_than(a,1),b,0),c)"), False)]
    assert q.columns() == ["g", "a", "b", "c"]
    hand = QueryContext(["g"], [("SUM", "CASE WHEN a > 1 THEN b ELSE 0 END"), ("MAX", "case(greater_than(a,1),b,0)")])
    assert hand.aggregations == [("SUM", "case(greater_than(a,1),b,0)"), ("MAX", "case(greater_than(a,1),b,0)")]
    assert list(hand.expressions) == ["case(greater_than(a,1),b,0)"]
    # (a nested CASE fits the stack as the ELSE, which is emitted first; as a THEN it stands above the ELSE: depth 5)
    nested = parse_expression("CASE WHEN a > 1 THEN 3 ELSE CASE WHEN b > 1 THEN 1 ELSE 2 END END")
    assert expr_name(nested) == "case(greater_than(a,1),3,case(greater_than(b,1),1,2))"


def test_case_on_a_predicates_left():
    q = parse_query("SELECT COUNT(*) FROM t WHERE g = 1 AND CASE WHEN a > 1 THEN b ELSE c END > 3", filter_expressions=True)
    leaf = q.filter.children[1].predicate
    assert leaf.column == "case(greater_than(a,1),b,c)" and leaf.values == ["3", "*"]
    assert list(q.expressions) == [leaf.column]
    with pytest.raises(ValueError):
        parse_query("SELECT COUNT(*) FROM t WHERE CASE WHEN a > 1 THEN b ELSE c END > 3")  # (off by default, as before)
    hand = QueryContext([], [("COUNT", "*")], Q.FilterContext.pred(Q.Predicate.eq("CASE WHEN a > 1 THEN b ELSE c END", 3)))
    assert hand.filter.predicate.column == leaf.column


# ------------------------------------------------------------------------------------------------ typing
@pytest.mark.parametrize("raw, text, typ", [
    ("0.1", "0.1", "FLOAT"), ("0.0", "0.0", "FLOAT"), ("2.5", "2.5", "FLOAT"), ("1.0E10", "1.0E10", "FLOAT"),
    ("16777217", "16777217", "INT"), ("2147483647", "2147483647", "INT"), ("2147483648", "2147483648", "LONG"),
    ("-2147483648", "-2147483648", "INT"), ("-2147483649", "-2147483649", "LONG"),
    ("9223372036854775807", "9223372036854775807", "LONG"),
    ("0.12345678", "0.12345678", "DOUBLE"),       # 8 decimals
    ("0.1234567", "0.1234567", "FLOAT"),          # 7
    ("1e39", "1.0E39", "DOUBLE"),                 # its float is infinite
    ("1e-46", "1.0E-46", "DOUBLE"),               # its float is zero
    ("12345678.5", "1.23456785E7", "DOUBLE"),     # 8 digits after the point of its E form
    ("123456.789012345", "123456.789012345", "DOUBLE"),
])
def test_literal_typing_table(raw, text, typ):
    assert Q.typed_literal_text(raw) == text
    assert Q.literal_type(text) == typ == C.lit_type(text)


@pytest.mark.parametrize("raw", ["0.12345678901234567", "1234567890.1234567", "9223372036854775808", "true", "false",
                                 "abc", "2020-01-01 00:00:00", "1e999"])
def test_declined_literals(raw):
    with pytest.raises(ValueError):
        Q.literal_type(Q.typed_literal_text(raw))


def test_result_type_of_every_pair():
    name = {"INT": "i", "LONG": "l", "FLOAT": "f", "DOUBLE": "d"}
    lit = {"INT": "1", "LONG": "2147483648", "FLOAT": "0.5", "DOUBLE": "0.12345678"}
    want = {frozenset(["INT"]): "INT", frozenset(["LONG"]): "LONG", frozenset(["FLOAT"]): "FLOAT",
            frozenset(["DOUBLE"]): "DOUBLE", frozenset(["INT", "LONG"]): "LONG"}
    cols = {"i": np.zeros(1, np.int32), "l": np.zeros(1, np.int64), "f": np.zeros(1, np.float32), "d": np.zeros(1), "j": np.zeros(1, np.int32)}
    for a in name:
        for b in name:
            r = want.get(frozenset([a, b]), "DOUBLE")
            for then, els in ((name[a], name[b]), (lit[a], name[b]), (name[a], lit[b]), (lit[a], lit[b])):
                t = parse_expression("CASE WHEN j > 0 THEN %s ELSE %s END" % (then, els))
                assert Q.expr_type(t, TYPES) == r == C.node_type(t, cols), (then, els)
    # folded over ELSE, then the THENs in order; an arithmetic node is DOUBLE; a nested CASE has its own R
    assert Q.expr_type(parse_expression("CASE WHEN j > 0 THEN 1 WHEN j > 1 THEN l ELSE i END"), TYPES) == "LONG"
    assert Q.expr_type(parse_expression("CASE WHEN j > 0 THEN 1 WHEN j > 1 THEN 0.5 ELSE i END"), TYPES) == "DOUBLE"
    assert Q.expr_type(parse_expression("CASE WHEN j > 0 THEN i + 1 ELSE 0 END"), TYPES) == "DOUBLE"
    assert Q.expr_type(parse_expression("CASE WHEN j > 0 THEN 0.25 ELSE CASE WHEN i > 0 THEN 0.5 ELSE f END END"), TYPES) == "FLOAT"


# ------------------------------------------------------------------------------------------------ programs
def test_select_order_and_literal_values():
    f = 0.10000000149011612  # (double)(float)0.1
    assert float(np.float32(0.1)) == f
    # all branches FLOAT: every literal is read as a float
    assert expr_program(parse_expression("CASE WHEN i > 1 THEN 0.1 ELSE 0.0 END"), TYPES) == \
        [(LIT, None, 0.0), (LIT, None, f), (COL, "i", 0.0), (LIT, None, 1.0), (L.EXPR_GT, None, 0.0), (SEL, None, 0.0)]
    # R = DOUBLE through the column: the plain double
    assert expr_program(parse_expression("CASE WHEN i > 1 THEN 0.1 ELSE d END"), TYPES)[:2] == [(COL, "d", 0.0), (LIT, None, 0.1)]
    assert expr_program(parse_expression("CASE WHEN i > 1 THEN 0.1 ELSE f END"), TYPES)[1] == (LIT, None, f)
    assert expr_program(parse_expression("CASE WHEN i > 1 THEN 0.1 ELSE i END"), TYPES)[1] == (LIT, None, 0.1)
    # a comparison's literal is read as its own type, whatever the other side is
    assert expr_program(parse_expression("CASE WHEN d > 0.1 THEN 1 ELSE 0 END"), TYPES)[3] == (LIT, None, f)
    assert expr_program(parse_expression("CASE WHEN d > 0.12345678 THEN 1 ELSE 0 END"), TYPES)[3] == (LIT, None, 0.12345678)
    assert expr_program(parse_expression("CASE WHEN d > 16777217 THEN 1 ELSE 0 END"), TYPES)[3] == (LIT, None, 16777217.0)
    # e, rN, cN, SELECT, .., r1, c1, SELECT: depth 4 for any number of WHENs over simple operands
    ops = expr_program(parse_expression("CASE WHEN i > 3 THEN 3 WHEN i > 2 THEN 2 WHEN i > 1 THEN 1 ELSE 0 END"), TYPES)
    assert [o[2] for o in ops if o[0] == LIT] == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0]
    assert [o[0] for o in ops].count(SEL) == 3 and len(ops) == 16
    assert _depth(ops) == 4
    with pytest.raises(ValueError):  # the values depend on the column types
        expr_program(parse_expression("CASE WHEN i > 1 THEN 0.1 ELSE 0.0 END"))
    assert expr_program(parse_expression("i * j")) == expr_program(parse_expression("i * j"), TYPES)  # arithmetic: as before


def _depth(ops):
    d = m = 0
    for op, _, _ in ops:
        d += 1 if op in (COL, LIT) else -2 if op == SEL else -1
        m = max(m, d)
    return m


def test_and_or_are_lowered_to_selects_within_depth_4():
    """Two comparisons joined by AND / OR stand above ELSE and THEN: a stack of 5 (test_and_or_need_a_stack_of_five).
    The program selects the same branch per doc with SELECTs only."""
    ops = expr_program(parse_expression("CASE WHEN i > 1 AND j < 2 THEN d ELSE e END"), TYPES)
    assert ops == [(COL, "e", 0.0), (COL, "d", 0.0), (COL, "j", 0.0), (LIT, None, 2.0), (L.EXPR_LT, None, 0.0), (SEL, None, 0.0),
                   (COL, "e", 0.0), (COL, "i", 0.0), (LIT, None, 1.0), (L.EXPR_LE, None, 0.0), (SEL, None, 0.0)]
    ops = expr_program(parse_expression("CASE WHEN i > 1 OR j < 2 THEN d ELSE e END"), TYPES)
    assert ops == [(COL, "e", 0.0), (COL, "d", 0.0), (COL, "j", 0.0), (LIT, None, 2.0), (L.EXPR_LT, None, 0.0), (SEL, None, 0.0),
                   (COL, "d", 0.0), (COL, "i", 0.0), (LIT, None, 1.0), (L.EXPR_GT, None, 0.0), (SEL, None, 0.0)]
    assert _depth(ops) == 4 and L.EXPR_AND not in [o[0] for o in ops]


# ------------------------------------------------------------------------------------------------ declined shapes
@pytest.mark.parametrize("sql", [
    "SELECT SUM(CASE WHEN a > 1 THEN b END) FROM t",                      # a missing ELSE
    "SELECT SUM(case(greater_than(a,1),b)) FROM t",
    "SELECT SUM(CASE WHEN a IN (1, 2) THEN b ELSE 0 END) FROM t",         # IN inside WHEN
    "SELECT SUM(CASE WHEN a NOT IN (1, 2) THEN b ELSE 0 END) FROM t",
    "SELECT SUM(CASE WHEN a BETWEEN 1 AND 2 THEN b ELSE 0 END) FROM t",
    "SELECT SUM(a > 5) FROM t",                                           # a boolean used as a number
    "SELECT SUM(greater_than(a, 5)) FROM t",
    "SELECT SUM(greater_than(a, 5) + 1) FROM t",
    "SELECT SUM(CASE WHEN a > 1 THEN b > 2 ELSE 0 END) FROM t",
    "SELECT SUM(case(greater_than(a,1),greater_than(b,2),0)) FROM t",
    "SELECT SUM(CASE WHEN a THEN b ELSE 0 END) FROM t",                   # a number used as a condition
    "SELECT SUM(case(a,b,0)) FROM t",
    "SELECT SUM(and(a, b)) FROM t",
    "SELECT SUM(CASE WHEN 1 > 0 THEN b ELSE 0 END) FROM t",               # a literal-only condition
    "SELECT SUM(CASE WHEN a = 'x' THEN b ELSE 0 END) FROM t",             # strings, booleans, timestamps
    "SELECT SUM(CASE WHEN a = true THEN b ELSE 0 END) FROM t",
    "SELECT SUM(CASE WHEN a > 1 THEN false ELSE 0 END) FROM t",
    "SELECT SUM(CASE WHEN ts > '2020-01-01 00:00:00' THEN b ELSE 0 END) FROM t",
    "SELECT SUM(CASE WHEN a > 0.12345678901234567 THEN b ELSE 0 END) FROM t",   # 17 significant digits
    "SELECT SUM(CASE WHEN a > 9223372036854775808 THEN b ELSE 0 END) FROM t",   # past int64
    "SELECT SUM(CASE a WHEN 1 THEN b ELSE 0 END) FROM t",                 # the simple form
    "SELECT SUM(a) FROM t GROUP BY CASE WHEN a > 1 THEN b ELSE 0 END",
])
def test_value_errors(sql):
    with pytest.raises(ValueError):
        q = parse_query(sql)
        for tree in q.expressions.values():  # (what only the column types can tell is declined with the program)
            expr_program(tree, {c: "INT" for c in expr_columns(tree)})


@pytest.mark.parametrize("expr", [
    "CASE WHEN l > 0.5 THEN 1 ELSE 0 END", "CASE WHEN l > d THEN 1 ELSE 0 END", "CASE WHEN f < l THEN 1 ELSE 0 END",
    "CASE WHEN d > 2147483648 THEN 1 ELSE 0 END", "CASE WHEN i * 2 > l THEN 1 ELSE 0 END",
    ("case", [("greater_than", [("case", [("greater_than", [("col", "i"), ("lit", "0")]), ("col", "l"), ("lit", "0")]),
                                ("lit", "0.5")]), ("lit", "1"), ("lit", "0")]),  # (by hand: it is past the stack too)
    "CASE WHEN s = 1 THEN 1 ELSE 0 END", "CASE WHEN i = 1 THEN s ELSE 0 END"])
def test_declined_by_the_column_types(expr):
    """A LONG side (column, literal, LONG-typed CASE) against a FLOAT or DOUBLE side; STRING operands."""
    with pytest.raises(ValueError) as e:
        expr_program(parse_expression(expr) if isinstance(expr, str) else expr, TYPES)
    assert "LONG" in str(e.value) or "STRING" in str(e.value)
    ok = parse_expression("CASE WHEN l > 2147483648 AND l >= i THEN 1 ELSE 0 END")  # LONG against LONG and INT is fine
    assert len(expr_program(ok, TYPES)) == 11


@pytest.mark.parametrize("expr, word", [
    ("CASE WHEN a > 4 THEN 4 WHEN a > 3 THEN 3 WHEN a > 2 THEN 2 WHEN a > 1 THEN 1 ELSE 0 END", "21 ops"),
    ("CASE WHEN a * b > c * d THEN 1 ELSE 0 END", "stack of 5"),
    ("a * b - CASE WHEN a > 1 THEN 1 ELSE 0 END", "stack of 5"),
    ("CASE WHEN a > 1 THEN b WHEN c > 1 THEN d ELSE e END", "5 columns"),
])
def test_limits_are_explained(expr, word):
    with pytest.raises(ValueError) as e:
        parse_expression(expr)
    assert word in str(e.value)


# ------------------------------------------------------------------------------------------------ case_check
def _run_check(lines):
    check = build.build_case_check()
    res = subprocess.run([check], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout.split("\n")


def _prog_lines(ops, index):
    out = ["prog %d" % len(ops)]
    for op, col, lit in ops:
        out.append("c %d" % index[col] if op == COL else "l %016x" % E.bits(lit) if op == LIT else "o %d" % op)
    return out


C0, C1, GT = ["c 0"], ["c 1"], ["o 8"]


@pytest.mark.parametrize("name, prog, code", [
    ("cmp_on_a_boolean", C0 + C1 + GT + C0 + GT, 9),
    ("arithmetic_on_a_boolean", C0 + C1 + GT + C0 + ["o 2"], 9),
    ("select_without_a_boolean_on_top", C0 + C1 + C0 + ["o 14"], 9),
    ("select_with_a_boolean_then", C0 + C0 + C1 + GT + C0 + C1 + GT + ["o 14"], 9),
    ("select_with_a_boolean_else", C0 + C1 + GT + C0 + C0 + C1 + GT + ["o 14"], 9),
    ("leaves_a_boolean", C0 + C1 + GT, 9),
    ("and_of_numbers", C0 + C1 + ["o 12"], 9),
    ("or_of_a_number_and_a_boolean", C0 + C0 + C1 + GT + ["o 13"], 9),
    ("select_underflow", C0 + C1 + GT + ["o 14"], 3),
    ("fifteen_is_unknown", C0 + C1 + ["o 15"], 2),
    ("and_needs_five", C0 + C1 + C0 + C1 + GT + C0 + C1, 4),
])
def test_badly_typed_programs_are_refused(name, prog, code):
    """expr_compile's verdict: what pgpu_table_add_expression answers PGPU_ERR_INVALID_ARGUMENT to."""
    got = _run_check(["prog %d" % len(prog)] + prog + ["rows 0"])
    assert got[0].startswith("error %d " % code), got[0]
    if code == 9:
        assert "bad operand type" in got[0]


def test_and_or_need_a_stack_of_five():
    """A boolean is only made above the ELSE and THEN its SELECT reads, so AND / OR of two comparisons need five
    entries: the well-typed program is refused for its depth alone, and the ops themselves work (the stack lines)."""
    prog = C0 + C1 + C0 + C1 + GT + C1 + C0 + GT + ["o 12", "o 14"]
    assert _run_check(["prog %d" % len(prog)] + prog + ["rows 0"])[0].startswith("error 4 ")
    one, zero, x, y = E.bits(1.0), E.bits(0.0), E.bits(2.5), E.bits(-7.0)
    lines, want = [], []
    for op, fn in ((12, lambda a, b: a and b), (13, lambda a, b: a or b)):
        for a in (0, 1):
            for b in (0, 1):
                lines.append("stack %d %016x %016x %016x %016x" % (op, (zero, one)[b], (zero, one)[a], x, y))
                want.append("%016x %016x %016x" % ((zero, one)[fn(a, b)], x, y))
    for c in (0, 1):  # SELECT: cond on top, then `then`, then `else`; two entries leave
        lines.append("stack 14 %016x %016x %016x %016x" % ((zero, one)[c], x, y, one))
        want.append("%016x %016x" % ((y, x)[c], one))
    # (the rows below those an op leaves are not specified: only the live ones are compared)
    assert [g[:len(w)] for g, w in zip(_run_check(lines), want)] == want


SPECIAL = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.1, 0.10000000149011612, 0.09999999999999999, 1.0,
           -1.0, 5e-324, -5e-324, 16777216.0, 16777217.0, 2.0 ** 53, 1e308]


def _random_case(rng, cols, types):
    """A random canonical tree over typed columns that the compiler accepts (None where it declines or the limits say
    no)."""
    def operand(kinds):
        k = kinds[rng.integers(len(kinds))]
        if k == "col":
            return ("col", cols[rng.integers(len(cols))])
        if k == "arith":
            fn = ("add", "sub", "mult", "div")[rng.integers(4)]
            return (fn, [("col", cols[rng.integers(len(cols))]), operand(["col", "alit"])])
        if k == "alit":
            return ("lit", repr(float(rng.choice([0.1, -2.5, 3.0, 0.0]))))
        return ("lit", str(rng.choice(["0", "1", "-3", "0.1", "0.0", "-0.0", "2.5", "0.12345678", "16777217", "1.0E10",
                                       "0.3", "1.0E-4"])))

    def comparison():
        fn = C.CMP[rng.integers(6)]
        return (fn, [operand(["col", "col", "arith"]), operand(["col", "lit", "lit"])])

    def condition():
        r = rng.random()
        if r < 0.6:
            return comparison()
        return (("and", "or")[rng.integers(2)], [comparison(), comparison()])
    n = int(rng.integers(1, 4))
    tree = ("case", [condition() for _ in range(n)] + [operand(["col", "lit", "lit", "arith"]) for _ in range(n + 1)])
    r = rng.random()
    if r < 0.15:
        tree = ("sub", [tree, ("col", cols[0])])
    elif r < 0.3:
        tree = ("mult", [tree, ("lit", "2.0")])
    try:
        Q.check_expr_limits(tree)
        expr_program(tree, types)
    except ValueError:
        return None
    return tree


def test_case_check_matches_the_typed_yardstick():
    rng = np.random.default_rng(17)
    ndocs = 40
    types = {"i": "INT", "j": "INT", "f": "FLOAT", "d": "DOUBLE", "e": "DOUBLE"}
    names = list(types)
    index = {c: k for k, c in enumerate(names)}
    cols = {"i": rng.integers(-3, 4, ndocs).astype(np.int32), "j": rng.integers(-3, 4, ndocs).astype(np.int32),
            "f": rng.choice([0.1, 0.3, -2.5, 0.0, 2.5], ndocs).astype(np.float32),
            "d": rng.choice(SPECIAL, ndocs), "e": rng.choice(SPECIAL, ndocs)}
    cols["d"][:len(SPECIAL)] = SPECIAL
    cols["e"][:len(SPECIAL)] = SPECIAL[::-1]
    n = len(SPECIAL)
    cols["d"][n:n + 4] = [0.0, -0.0, float("nan"), float("nan")]
    cols["e"][n:n + 4] = [-0.0, 0.0, float("nan"), float("inf")]
    trees = [parse_expression(s) for s in (
        "CASE WHEN d = e THEN 1 ELSE 0 END", "CASE WHEN d > e THEN 1 WHEN d < e THEN -1 ELSE 0 END",
        "CASE WHEN d >= 0.0 THEN 1 ELSE 0 END", "CASE WHEN d = 0.1 THEN 0.1 ELSE 0.0 END",
        "CASE WHEN d > 0.1 AND e <= 0.1 THEN d ELSE e END", "CASE WHEN f = 0.1 OR i > j THEN f ELSE 0.3 END",
        "CASE WHEN e > 0 THEN d / e ELSE 0 END", "CASE WHEN i = 1 THEN 16777217 ELSE f END")]
    tried = 0
    while len(trees) < 3000 and tried < 40000:
        tried += 1
        t = _random_case(rng, names, types)
        if t is not None:
            trees.append(t)
    assert len(trees) == 3000
    lines, want = [], []
    for t in trees:
        ops = expr_program(t, types)
        used = []
        for op, c, _ in ops:
            if op == COL and c not in used:
                used.append(c)
        lines += _prog_lines(ops, index) + ["rows %d" % ndocs]
        lines += [" ".join("%016x" % E.bits(float(cols[c][k])) for c in used) for k in range(ndocs)]
        vals = C.eval_docs(t, cols).tolist()
        want.append("ok %d" % len(used))
        want += ["%016x %d" % (E.canon_bits(v), E.key(v)) for v in vals]
    got = _run_check(lines)
    got = [" ".join(g.split()[:2]) if g.startswith("ok") else g if not g else
           "%016x %s" % (E.canon_bits(E.from_bits(int(g.split()[0], 16))), g.split()[1]) for g in got]
    assert got[:len(want)] == want
    # the specials count: -0.0 = 0.0 is false and NaN = NaN true under Double.compare, unlike ==
    eq = C.eval_docs(trees[0], cols)
    d, e = cols["d"], cols["e"]
    assert any(eq[k] == 0.0 and d[k] == e[k] for k in range(ndocs))
    assert any(eq[k] == 1.0 and d[k] != d[k] for k in range(ndocs))
    gt = C.eval_docs(trees[1], cols)
    assert any(gt[k] == 1.0 and d[k] != d[k] and e[k] == float("inf") for k in range(ndocs)) or \
        any(gt[k] == -1.0 and e[k] != e[k] for k in range(ndocs))


def test_compared_columns_are_reported():
    """The mask the plan reads to find LONG columns whose values reach a comparison as they are."""
    index = {"a": 0, "b": 1, "c": 2}
    types = {"a": "LONG", "b": "LONG", "c": "LONG"}
    for expr, mask in (("CASE WHEN a > 1 THEN b ELSE c END", 0b100),                 # first use: c, b, a
                       ("CASE WHEN a + 1 > 1 THEN b ELSE c END", 0),
                       ("CASE WHEN a > b THEN a - b ELSE 0 END", 0b011)):
        ops = expr_program(parse_expression(expr), types)
        got = _run_check(_prog_lines(ops, index) + ["rows 0"])
        assert got[0].split()[2] == str(mask), (expr, got[0])
