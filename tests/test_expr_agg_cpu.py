"""Expressions inside aggregations, without a GPU: the Python layer's normalisation (one canonical tree, program and
function-form name per expression; every ValueError) and the host build of the shared evaluator (tools/expr_check.cpp
over pinot_amd/csrc/expr_eval.h, under AddressSanitizer + UndefinedBehaviorSanitizer with contraction off) against the
Python-float yardstick of expr_common.py: same bits, same keys."""
import subprocess

import numpy as np
import pytest

import expr_common as E
from pinot_amd import _lib as L
from pinot_amd import build
from pinot_amd.query import QueryContext, expr_columns, expr_name, expr_program, parse_expression, parse_query

COL, LIT, ADD, SUB, MULT, DIV = L.EXPR_COLUMN, L.EXPR_LITERAL, L.EXPR_ADD, L.EXPR_SUB, L.EXPR_MULT, L.EXPR_DIV


# ------------------------------------------------------------------------------------------------ normalisation
def test_spellings_share_one_tree_program_and_name():
    qs = [parse_query("SELECT SUM(%s) FROM t GROUP BY g" % s)
          for s in ("a*b", "MULT(a,b)", "times(a,b)", "mult( a , b )", "(a * b)", "Times(a, b)")]
    for q in qs:
        assert q.aggregations == [("SUM", "mult(a,b)")]
        assert q.expressions == {"mult(a,b)": ("mult", [("col", "a"), ("col", "b")])}
        assert expr_program(q.expressions["mult(a,b)"]) == \
            [(LIT, None, 1.0), (COL, "a", 0.0), (MULT, None, 0.0), (COL, "b", 0.0), (MULT, None, 0.0)]
    assert QueryContext(["g"], [("SUM", "a * b")]).aggregations == [("SUM", "mult(a,b)")]
    assert QueryContext(["g"], [("SUM", "mult(a,b)")]).expressions == qs[0].expressions
    for alias, fn in (("PLUS", "add"), ("MINUS", "sub"), ("TIMES", "mult"), ("DIVIDE", "div")):
        assert expr_name(parse_expression("%s(a, b)" % alias)) == "%s(a,b)" % fn


def test_nary_add_folds_its_literals_first():
    tree = parse_expression("ADD(a, 0.1, b, 0.2)")
    assert expr_name(tree) == "add(a,0.1,b,0.2)"
    assert expr_program(tree) == [(LIT, None, 0.0 + 0.1 + 0.2), (COL, "a", 0.0), (ADD, None, 0.0), (COL, "b", 0.0),
                                  (ADD, None, 0.0)]
    # the leading 0.0 + is there without a literal too: ADD(x, y) of two -0.0 is +0.0
    assert expr_program(parse_expression("a + b"))[0] == (LIT, None, 0.0)
    assert E.bits(E.eval_tree(parse_expression("a + b"), {"a": -0.0, "b": -0.0})) == E.bits(0.0)
    assert E.bits(E.eval_tree(parse_expression("a - b"), {"a": -0.0, "b": 0.0})) == E.bits(-0.0)
    mult = parse_expression("MULT(2, a, 0.5, b)")
    assert expr_program(mult)[0] == (LIT, None, 1.0 * 2.0 * 0.5)


def test_precedence_parentheses_and_unary_minus():
    assert expr_name(parse_expression("a + b * c")) == "add(a,mult(b,c))"
    assert expr_name(parse_expression("(a + b) * c")) == "mult(add(a,b),c)"
    assert expr_name(parse_expression("a - b - c")) == "sub(sub(a,b),c)"
    assert expr_name(parse_expression("a / b * c")) == "mult(div(a,b),c)"
    assert expr_name(parse_expression("a-1")) == "sub(a,1.0)"
    assert expr_name(parse_expression("a * -2.5")) == "mult(a,-2.5)"
    assert expr_name(parse_expression("ADD(DIV(a,b), DIV(c,d))")) == "add(div(a,b),div(c,d))"
    assert expr_name(parse_expression("add(div(a,b),2.5)")) == "add(div(a,b),2.5)"
    assert expr_columns(parse_expression("a*b + b*c/a")) == ["a", "b", "c"]
    q = parse_query("SELECT SUM(a*b), COUNT(*), MAX(a*b), SUM(a), AVG(times(a, b)), MIN(c-d) FROM t WHERE f < -3 "
                    "GROUP BY g ORDER BY SUM(a*b) DESC LIMIT 3")
    assert q.aggregations == [("SUM", "mult(a,b)"), ("COUNT", "*"), ("MAX", "mult(a,b)"), ("SUM", "a"),
                              ("AVG", "mult(a,b)"), ("MIN", "sub(c,d)")]
    assert sorted(q.expressions) == ["mult(a,b)", "sub(c,d)"]  # equal expressions share one entry
    assert q.order_by == [(("agg", "SUM", "mult(a,b)"), False)] and q.limit == 3
    assert q.columns() == ["f", "g", "a", "b", "c", "d"]
    assert q.filter.predicate.values == ["*", "-3"]  # (a number's sign is a token of its own; a literal takes it back)
    plain = parse_query("SELECT SUM(a), COUNT(*) FROM t WHERE a BETWEEN -5 AND 5 GROUP BY g")
    assert plain.expressions == {} and plain.aggregations == [("SUM", "a"), ("COUNT", "*")]
    assert plain.filter.predicate.values == ["-5", "5"]


@pytest.mark.parametrize("sql", [
    "SELECT SUM(SUB(a, b, c)) FROM t", "SELECT SUM(SUB(a)) FROM t", "SELECT SUM(DIV(a, b, c)) FROM t",
    "SELECT SUM(DIVIDE(a)) FROM t", "SELECT SUM(ADD(a)) FROM t", "SELECT SUM(MULT(a)) FROM t",
    "SELECT SUM(1 + 2) FROM t", "SELECT SUM(ADD(1, 2.5)) FROM t", "SELECT SUM(a + MULT(2, 3)) FROM t",
    "SELECT SUM(FOO(a, b)) FROM t", "SELECT SUM(POW(a, 2)) FROM t", "SELECT SUM(-a) FROM t",
    "SELECT SUM(a) FROM t GROUP BY a + b", "SELECT SUM(a) FROM t GROUP BY ADD(a, b)", "SELECT SUM(a) FROM t GROUP BY g, a*b",
    "SELECT SUM(a) FROM t WHERE a * b > 3", "SELECT SUM(a) FROM t WHERE ADD(a, b) > 3", "SELECT SUM(a) FROM t WHERE g = 1 AND a + b < 3",
])
def test_value_errors(sql):
    with pytest.raises(ValueError):
        parse_query(sql)


@pytest.mark.parametrize("sql, word", [
    ("SELECT SUM(a + b + c + d + e) FROM t", "17 ops"),          # four nested binary nodes, a folded literal each
    ("SELECT SUM(a*b + c*d + e*f) FROM t", "21 ops"),
    ("SELECT SUM(a / (b / (c / (d / (a / b))))) FROM t", "stack of 6"),
    ("SELECT SUM(ADD(a, b, c, d, e)) FROM t", "5 columns"),
])
def test_limits_are_explained_by_the_python_layer(sql, word):
    with pytest.raises(ValueError) as e:
        parse_query(sql)
    assert word in str(e.value)


def test_the_nary_form_fits_where_the_infix_chain_does_not():
    q = parse_query("SELECT SUM(ADD(a, b, c, d, 1, 2)), SUM(a + b + c + d) FROM t")
    assert [len(expr_program(t)) for t in q.expressions.values()] == [9, 13]


def test_quoted_identifiers_stay_columns():
    q = parse_query('SELECT SUM("a-b"), SUM(a-b), MAX("x(1)" * 2) FROM t GROUP BY "g/h"')
    assert q.aggregations == [("SUM", "a-b"), ("SUM", "sub(a,b)"), ("MAX", "mult(x(1),2.0)")]
    assert sorted(q.expressions) == ["mult(x(1),2.0)", "sub(a,b)"] and q.group_by == ["g/h"]
    assert q.columns() == ["g/h", "a-b", "a", "b", "x(1)"]
    # built by hand: `expressions` given says which arguments are expressions, every other name is a column
    assert QueryContext(["g/h"], [("SUM", "a-b")], expressions={}).aggregations == [("SUM", "a-b")]


def test_query_context_value_errors():
    with pytest.raises(ValueError):
        QueryContext(["a+b"], [("SUM", "a")])
    with pytest.raises(ValueError):
        QueryContext([], [("SUM", "SUB(a,b,c)")])
    with pytest.raises(ValueError):
        QueryContext([], [("SUM", "2 * 3")])
    with pytest.raises(KeyError):  # an expression is a column only once a table has registered it
        QueryContext([], [("SUM", "a*b")]).to_c({"a": 0, "b": 1})
    c, keep = QueryContext([], [("COUNT", "a*b"), ("SUM", "a")]).to_c({"a": 0, "b": 1})
    assert (c.aggs[0].fn, c.aggs[0].column) == (L.AGG_COUNT, -1)  # COUNT(expr) is COUNT
    c, keep = QueryContext([], [("SUM", "a*b")]).to_c({"a": 0, "b": 1, "mult(a,b)": 2})
    assert (c.aggs[0].fn, c.aggs[0].column) == (L.AGG_SUM, 2)


# ------------------------------------------------------------------------------------------------ expr_check
def _random_tree(rng, cols, budget):
    """A random canonical tree of at most `budget` program ops (its own count returned too)."""
    def leaf():
        if rng.random() < 0.8:
            return ("col", cols[rng.integers(len(cols))])
        return ("lit", repr(float(rng.choice([0.1, -2.5, 3.0, 1e-3, 7.25, -0.0]))))
    fn = ("add", "sub", "mult", "div")[rng.integers(4)]
    n = 2 if fn in ("sub", "div") else int(rng.integers(2, 4))
    args = []
    for _ in range(n):
        args.append(_random_tree(rng, cols, budget // 2) if budget >= 12 and rng.random() < 0.4 else leaf())
    if not any(expr_columns(a) for a in args):
        args[0] = ("col", cols[0])
    return (fn, args)


def _depth(ops):
    d = m = 0
    for op, _, _ in ops:
        d += 1 if op in (COL, LIT) else -1
        m = max(m, d)
    return m


def _block(ops, index, rows):
    lines = ["prog %d" % len(ops)]
    for op, col, lit in ops:
        lines.append("c %d" % index[col] if op == COL else "l %016x" % E.bits(lit) if op == LIT else "asmd"[op - ADD])
    lines.append("rows %d" % len(rows))
    lines += [" ".join("%016x" % E.bits(x) for x in r) for r in rows]
    return lines


def _run_check(lines):
    check = build.build_expr_check()
    res = subprocess.run([check], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout.split("\n")


def test_expr_check_matches_python_floats():
    rng = np.random.default_rng(11)
    cols = ["a", "b", "c", "d", "e", "f"]
    index = {c: i for i, c in enumerate(cols)}
    ndocs = 24
    # full-mantissa doubles (a fused multiply-add rounds differently on most of them), and the special values
    data = {c: rng.uniform(-2.0, 2.0, ndocs) for c in cols}
    data["a"][:4] = [0.0, -0.0, 1e308, -1e-310]
    data["b"][:4] = [-0.0, 0.0, 1e10, 3.0]
    data["c"][:4] = [0.0, -0.0, float("inf"), float("nan")]
    assert sum(E.fused_differs(a, b, c) for a, b, c in zip(data["a"], data["b"], data["c"])
               if np.isfinite([a, b, c]).all()) >= 1
    trees = [parse_expression(s) for s in ("a*b + c", "ADD(MULT(a,b), c)", "a/b", "a/c", "c - a*b", "ADD(DIV(a,b), DIV(c,d))",
                                            "a + b", "SUB(MULT(a, b), b)", "2.5 - a/-3", "ADD(a, 0.1, b, 0.2)")]
    while len(trees) < 300:
        t = _random_tree(rng, cols, 16)
        ops = expr_program(t)
        if len(ops) <= L.EXPR_MAX_OPS and _depth(ops) <= L.EXPR_MAX_DEPTH and len(expr_columns(t)) <= L.EXPR_MAX_COLUMNS:
            trees.append(t)
    lines, want = [], []
    for t in trees:
        used = expr_columns(t)
        rows = [[data[c][i] for c in used] for i in range(ndocs)]
        lines += _block(expr_program(t), index, rows)
        vals = [E.eval_tree(t, {c: float(data[c][i]) for c in used}) for i in range(ndocs)]
        want.append("ok %d" % len(used))
        want += ["%016x %d" % (E.canon_bits(v), E.key(v)) for v in vals]
    got = _run_check(lines)
    # (the printed bits are the machine's: a NaN is compared as the canonical one, expr_common.canon_bits)
    got = [g if g.startswith("ok") or not g else
           "%016x %s" % (E.canon_bits(E.from_bits(int(g.split()[0], 16))), g.split()[1]) for g in got]
    assert got[:len(want)] == want
    assert any(" %d" % E.key(float("nan")) in w for w in want)  # a NaN result takes the canonical NaN key
    assert any(w.startswith("%016x " % E.bits(float("inf"))) for w in want)  # x / 0 is inf


@pytest.mark.parametrize("name, prog, code", [
    ("stack_underflow", ["c 0", "a"], 3),
    ("two_values_left", ["c 0", "c 1"], 6),
    ("seventeen_ops", ["c 0"] + ["c 1", "a"] * 8, 1),
    ("depth_five", ["c 0", "c 1", "c 2", "c 3", "c 0", "a", "a", "a", "a"], 4),
    ("five_columns", ["c 0", "c 1", "a", "c 2", "a", "c 3", "a", "c 4", "a"], 5),
    ("no_column", ["l 3ff0000000000000", "l 3ff0000000000000", "a"], 7),
    ("unknown_op", ["c 0", "c 1", "x"], 2),
    ("empty", [], 1),
])
def test_malformed_programs_are_refused(name, prog, code):
    """Each is what pgpu_table_add_expression answers PGPU_ERR_INVALID_ARGUMENT to: expr_compile's verdict."""
    got = _run_check(["prog %d" % len(prog)] + prog + ["rows 0"])
    assert got[0].startswith("error %d " % code), got[0]


def test_the_limits_themselves_are_accepted():
    """15 ops -- the longest well-formed program within 16 (k operands take k - 1 binary ops) -- at depth 4 over 4
    columns."""
    got = _run_check(["prog 15", "c 0", "c 1", "c 2", "c 3", "a", "a", "a"] + ["c 0", "m", "c 1", "s", "c 2", "d"] +
                     ["l 4000000000000000", "m", "rows 1", " ".join("%016x" % E.bits(x) for x in (1.5, 2.5, 3.5, 4.5))])
    assert got[0] == "ok 4"
    v = ((((1.5 + (2.5 + (3.5 + 4.5))) * 1.5) - 2.5) / 3.5) * 2.0
    assert got[1] == "%016x %d" % (E.bits(v), E.key(v))
