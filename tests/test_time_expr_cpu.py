"""Math and time functions in expressions, without a GPU: the parser's spellings, the emitted programs (the lowering of
TIMECONVERT and DATETIMECONVERT to long arithmetic), names and types, every decline by its message, the limits, the LONG
literal rule of a WHERE leaf, expr_compile's verdicts for the new ops (tools/case_check.cpp, the host entry of the older
ops' verdicts), the host check of the ops themselves (tools/math_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer) and the reference's known answers (tests/golden/kat_datetime_convert.json) through a
pure-Python interpreter of the emitted programs (tests/time_common.py)."""
import subprocess

import pytest

import time_common as T
from pinot_amd import _lib as L
from pinot_amd import build
from pinot_amd.query import (QueryContext, expr_columns, expr_name, expr_program, expr_type, long_literal_text,
                             parse_expression, parse_query, time_chain)

COL, LIT, MULT, DIV, LDIV, MOD = L.EXPR_COLUMN, L.EXPR_LITERAL, L.EXPR_MULT, L.EXPR_DIV, L.EXPR_LDIV, L.EXPR_MOD
TYPES = {"ts": "LONG", "days": "INT", "d": "DOUBLE", "f": "FLOAT", "i": "INT", "l": "LONG", "g": "INT", "s": "STRING",
         "DaysSinceEpoch": "INT", "price": "DOUBLE", "qty": "INT", "id": "INT"}


def _chain(col, *steps):
    """col, then LITERAL n, MULT / LDIV per step."""
    ops = [(COL, col, 0.0)]
    for kind, n in steps:
        ops += [(LIT, None, float(n)), (MULT if kind == "mult" else LDIV, None, 0.0)]
    return ops


# ------------------------------------------------------------------------------------------------ the op codes
def test_op_codes_follow_select_and_leave_15_unknown():
    assert L.EXPR_SELECT == 14
    assert (L.EXPR_ABS, L.EXPR_CEIL, L.EXPR_FLOOR, L.EXPR_SQRT, L.EXPR_MOD, L.EXPR_LDIV) == (16, 17, 18, 19, 20, 21)


# ------------------------------------------------------------------------------------------------ spellings
@pytest.mark.parametrize("spellings, name", [
    (("timeConvert(ts,'DAYS','SECONDS')", "TIMECONVERT(ts, 'DAYS', 'SECONDS')", "time_convert(ts,'DAYS','SECONDS')",
      "Time_Convert( ts ,'DAYS','SECONDS')", "TIME_CONVERT(ts,'DAYS','SECONDS')"), "timeconvert(ts,'DAYS','SECONDS')"),
    (("dateTimeConvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')",
      "DATE_TIME_CONVERT(ts, '1:MILLISECONDS:EPOCH', '1:HOURS:EPOCH', '1:HOURS')",
      "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')",
      "Date_Time_Convert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')"),
     "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')"),
    (("floor(d)", "FLOOR(d)", "Floor( d )"), "floor(d)"),
    (("ABS(d)", "abs(d)"), "abs(d)"), (("CEIL(d)", "ceil(d)"), "ceil(d)"), (("SQRT(d)", "Sqrt(d)"), "sqrt(d)"),
    (("MOD(i, 7)", "mod(i,7)", "Mod(i, 7.0)"), "mod(i,7.0)"),
])
def test_every_spelling_is_one_tree(spellings, name):
    trees = [parse_expression(s) for s in spellings]
    assert all(t == trees[0] for t in trees)
    assert expr_name(trees[0]) == name
    assert all(expr_program(t, TYPES) == expr_program(trees[0], TYPES) for t in trees)


def test_units_are_read_in_any_case_and_named_as_written():
    a, b = parse_expression("timeconvert(ts,'days','Seconds')"), parse_expression("timeconvert(ts,'DAYS','SECONDS')")
    assert expr_program(a, TYPES) == expr_program(b, TYPES) == _chain("ts", ("mult", 86400))
    assert expr_name(a) == "timeconvert(ts,'days','Seconds')"  # (the reference prints the literal as written)


def test_nesting_in_arithmetic_case_and_queries():
    t = parse_expression("DIV(timeConvert(DaysSinceEpoch,'DAYS','SECONDS'),1)")
    assert expr_name(t) == "div(timeconvert(DaysSinceEpoch,'DAYS','SECONDS'),1.0)"
    assert expr_program(t, TYPES) == _chain("DaysSinceEpoch", ("mult", 86400)) + [(LIT, None, 1.0), (DIV, None, 0.0)]
    assert expr_type(t, TYPES) == "DOUBLE"
    t = parse_expression("price * floor(qty / 10)")
    assert expr_name(t) == "mult(price,floor(div(qty,10.0)))"
    assert expr_program(t, TYPES) == [(LIT, None, 1.0), (COL, "price", 0.0), (MULT, None, 0.0), (COL, "qty", 0.0),
                                      (LIT, None, 10.0), (DIV, None, 0.0), (L.EXPR_FLOOR, None, 0.0), (MULT, None, 0.0)]
    t = parse_expression("CASE WHEN mod(id, 2) = 0 THEN price ELSE 0 END")
    assert expr_name(t) == "case(equals(mod(id,2.0),0),price,0)"
    assert expr_program(t, TYPES) == [(LIT, None, 0.0), (COL, "price", 0.0), (COL, "id", 0.0), (LIT, None, 2.0), (MOD, None, 0.0),
                                      (LIT, None, 0.0), (L.EXPR_EQ, None, 0.0), (L.EXPR_SELECT, None, 0.0)]
    t = parse_expression("CASE WHEN timeconvert(ts,'MILLISECONDS','DAYS') >= 17000 THEN 1 ELSE 0 END")
    assert expr_program(t, TYPES)[2:6] == _chain("ts", ("ldiv", 86400000)) + [(LIT, None, 17000.0)]
    t = parse_expression("sqrt(abs(d)) + ceil(f)")
    assert expr_name(t) == "add(sqrt(abs(d)),ceil(f))" and expr_columns(t) == ["d", "f"]
    q = parse_query("SELECT COUNT(*), MAX(timeConvert(DaysSinceEpoch,'DAYS','SECONDS')) FROM t WHERE "
                    "timeConvert(DaysSinceEpoch,'DAYS','SECONDS') IN (1388534400, 1391126400) AND g = 1 GROUP BY "
                    "dateTimeConvert(DaysSinceEpoch,'1:DAYS:EPOCH','1:HOURS:EPOCH','1:HOURS') ORDER BY "
                    "DATE_TIME_CONVERT(DaysSinceEpoch,'1:DAYS:EPOCH','1:HOURS:EPOCH','1:HOURS') LIMIT 5",
                    filter_expressions=True, group_by_expressions=True)
    bucket = "datetimeconvert(DaysSinceEpoch,'1:DAYS:EPOCH','1:HOURS:EPOCH','1:HOURS')"
    tc = "timeconvert(DaysSinceEpoch,'DAYS','SECONDS')"
    assert q.group_by == [bucket] and q.order_by == [(("col", bucket), True)]
    assert q.aggregations == [("COUNT", "*"), ("MAX", tc)]
    assert sorted(q.expressions) == sorted([bucket, tc])
    assert q.filter.children[0].predicate.column == tc and q.filter.children[0].predicate.values == ["1388534400", "1391126400"]
    assert q.columns() == ["DaysSinceEpoch", "g"]
    # a query built by hand reads the same text
    assert QueryContext(["g"], [("MAX", "time_convert(ts, 'DAYS', 'SECONDS')")]).aggregations == [("MAX", "timeconvert(ts,'DAYS','SECONDS')")]


# ------------------------------------------------------------------------------------------------ the lowering
MS, H, D, W = 1, 3600000, 86400000, 604800000
LOWERINGS = [
    # the reference's five epoch formats of DateTimeConverterTest, and millis -> WEEKS
    ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')", [("ldiv", 900000), ("mult", 900000)]),
    ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','1:MILLISECONDS')", []),
    ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')", [("ldiv", H), ("mult", H), ("ldiv", H)]),
    ("datetimeconvert(ts,'5:MINUTES:EPOCH','1:HOURS:EPOCH','1:HOURS')", [("mult", 300000), ("ldiv", H), ("mult", H), ("ldiv", H)]),
    ("datetimeconvert(ts,'5:MINUTES:EPOCH','1:MILLISECONDS:EPOCH','1:HOURS')", [("mult", 300000), ("ldiv", H), ("mult", H)]),
    ("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:WEEKS:EPOCH','1:MILLISECONDS')", [("ldiv", W)]),
    # a NANOSECONDS input: toMillis divides
    ("datetimeconvert(ts,'1:NANOSECONDS:EPOCH','1:SECONDS:EPOCH','1:SECONDS')",
     [("ldiv", 1000000), ("ldiv", 1000), ("mult", 1000), ("ldiv", 1000)]),
    # the worst case, 13 ops: no step is by 1 and no two multiplications meet
    ("datetimeconvert(ts,'7:NANOSECONDS:EPOCH','3:DAYS:EPOCH','5:MINUTES')",
     [("mult", 7), ("ldiv", 1000000), ("ldiv", 300000), ("mult", 300000), ("ldiv", D), ("ldiv", 3)]),
    # x * n and toMillis fold, and so do * G and a MICROSECONDS output's * 1000
    ("datetimeconvert(ts,'2:DAYS:EPOCH','1:DAYS:EPOCH','1:DAYS')", [("mult", 2 * D), ("ldiv", D), ("mult", D), ("ldiv", D)]),
    ("datetimeconvert(ts,'1:SECONDS:EPOCH','10:MICROSECONDS:EPOCH','1:MINUTES')",
     [("mult", 1000), ("ldiv", 60000), ("mult", 60000 * 1000), ("ldiv", 10)]),
    # timeconvert: one multiplication, one division, nothing; WEEKS through the milliseconds
    ("timeconvert(ts,'DAYS','SECONDS')", [("mult", 86400)]),
    ("timeconvert(ts,'MILLISECONDS','DAYS')", [("ldiv", D)]),
    ("timeconvert(ts,'HOURS','HOURS')", []),
    ("timeconvert(ts,'DAYS','NANOSECONDS')", [("mult", 86400 * 10 ** 9)]),
    ("timeconvert(ts,'NANOSECONDS','DAYS')", [("ldiv", 86400 * 10 ** 9)]),
    ("timeconvert(ts,'MILLISECONDS','WEEKS')", [("ldiv", W)]),
    ("timeconvert(ts,'DAYS','WEEKS')", [("mult", D), ("ldiv", W)]),
    ("timeconvert(ts,'MICROSECONDS','WEEKS')", [("ldiv", 1000), ("ldiv", W)]),
]


@pytest.mark.parametrize("text, steps", LOWERINGS)
def test_the_emitted_program(text, steps):
    tree = parse_expression(text)
    assert time_chain(tree) == steps
    ops = expr_program(tree, TYPES)
    assert ops == _chain("ts", *steps) and len(ops) == 1 + 2 * len(steps) <= 13
    assert expr_program(tree, TYPES) == ops and expr_program(parse_expression(text.upper().replace("TS", "ts")), TYPES) == ops
    assert expr_name(tree) == text and expr_type(tree, TYPES) == "LONG"
    assert expr_type(tree, {"ts": "INT"}) == "LONG"


def test_names_and_types():
    for text in ("abs(d)", "ceil(i)", "floor(l)", "sqrt(f)", "mod(i,2.0)", "mod(2.0,i)", "floor(div(qty,10.0))"):
        t = parse_expression(text)
        assert expr_name(t) == text and expr_type(t, TYPES) == "DOUBLE"
    # a CASE folds them: LONG and INT give LONG, LONG and DOUBLE give DOUBLE
    t = parse_expression("CASE WHEN i > 1 THEN timeconvert(ts,'DAYS','SECONDS') ELSE 0 END")
    assert expr_type(t, TYPES) == "LONG"
    t = parse_expression("CASE WHEN i > 1 THEN timeconvert(ts,'DAYS','SECONDS') ELSE floor(d) END")
    assert expr_type(t, TYPES) == "DOUBLE"
    # a LONG side against a FLOAT or DOUBLE side stays declined
    for cond in ("timeconvert(ts,'DAYS','SECONDS') > d", "timeconvert(ts,'DAYS','SECONDS') > 1.5", "floor(d) > l"):
        with pytest.raises(ValueError) as e:
            expr_program(parse_expression("CASE WHEN %s THEN 1 ELSE 0 END" % cond), TYPES)
        assert "LONG" in str(e.value)
    ok = parse_expression("CASE WHEN timeconvert(ts,'DAYS','SECONDS') > 86400 THEN 1 ELSE 0 END")
    assert len(expr_program(ok, TYPES)) == 8


# ------------------------------------------------------------------------------------------------ declines
@pytest.mark.parametrize("text, word", [
    ("exp(d)", "EXP is not supported"), ("LN(d)", "LN is not supported"), ("pow(d, 2)", "unknown function"),
    ("floor(3)", "FLOOR of the literal"), ("abs(-1.5)", "ABS of the literal"), ("sqrt(d, d)", "SQRT takes exactly 1 argument"),
    ("ceil()", None), ("mod(d)", "MOD takes exactly 2 arguments"), ("mod(d, 1, 2)", "MOD takes exactly 2 arguments"),
    ("mod(2, 3)", "literal-only"), ("d % 3", None),
    ("timeconvert(ts,'DAYS')", "TIMECONVERT takes exactly 3 arguments"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:DAYS:EPOCH')", "DATETIMECONVERT takes exactly 4 arguments"),
    ("timeconvert(ts + 1,'DAYS','SECONDS')", "first argument is an INT or LONG column"),
    ("timeconvert(floor(d),'DAYS','SECONDS')", "first argument is an INT or LONG column"),
    ("datetimeconvert(timeconvert(ts,'DAYS','HOURS'),'1:HOURS:EPOCH','1:DAYS:EPOCH','1:DAYS')", "first argument is an INT or LONG column"),
    ("datetimeconvert(ts,'1:DAYS:SIMPLE_DATE_FORMAT:yyyyMMdd','1:DAYS:EPOCH','1:DAYS')", "SIMPLE_DATE_FORMAT"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:DAYS:SIMPLE_DATE_FORMAT:yyyyMMdd','1:DAYS')", "SIMPLE_DATE_FORMAT"),
    ("timeconvert(ts,'DAYS','MONTHS')", "MONTHS as the output unit"), ("timeconvert(ts,'DAYS','YEARS')", "YEARS as the output unit"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:MONTHS:EPOCH','1:DAYS')", "MONTHS as the output unit"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:YEARS:EPOCH','1:DAYS')", "YEARS as the output unit"),
    ("timeconvert(ts,'WEEKS','DAYS')", "WEEKS as the input unit"), ("timeconvert(ts,'MONTHS','DAYS')", "MONTHS as the input unit"),
    ("datetimeconvert(ts,'1:WEEKS:EPOCH','1:DAYS:EPOCH','1:DAYS')", "WEEKS as the input unit"),
    ("datetimeconvert(ts,'1:YEARS:EPOCH','1:DAYS:EPOCH','1:DAYS')", "YEARS as the input unit"),
    ("timeconvert(ts,'FORTNIGHTS','DAYS')", "unknown time unit"),
    ("datetimeconvert(ts,'0:DAYS:EPOCH','1:DAYS:EPOCH','1:DAYS')", "not a positive integer"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','-2:DAYS:EPOCH','1:DAYS')", "not a positive integer"),
    ("datetimeconvert(ts,'1.5:DAYS:EPOCH','1:DAYS:EPOCH','1:DAYS')", "not a positive integer"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:DAYS:EPOCH','0:DAYS')", "not a positive integer"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:DAYS:EPOCH','x:DAYS')", "not a positive integer"),
    ("datetimeconvert(ts,'1:DAYS','1:DAYS:EPOCH','1:DAYS')", "no format"),
    ("datetimeconvert(ts,'1:DAYS:EPOCH','1:DAYS:EPOCH','DAYS')", "no granularity"),
    ("timeconvert(ts, d, 'DAYS')", "no string literal"), ("add(ts, 'DAYS')", None),
])
def test_declines(text, word):
    with pytest.raises(ValueError) as e:
        parse_expression(text)
    if word is not None:
        assert word in str(e.value), str(e.value)


def test_a_float_or_double_first_argument_is_declined_where_the_types_are_known():
    for col in ("d", "f"):
        tree = parse_expression("timeconvert(%s,'DAYS','SECONDS')" % col)
        with pytest.raises(ValueError) as e:
            expr_program(tree, TYPES)
        assert "first argument is an INT or LONG column" in str(e.value)
        tree = parse_expression("datetimeconvert(%s,'1:DAYS:EPOCH','1:HOURS:EPOCH','1:HOURS')" % col)
        with pytest.raises(ValueError):
            expr_program(tree, TYPES)
    with pytest.raises(ValueError):
        expr_program(parse_expression("timeconvert(s,'DAYS','SECONDS')"), TYPES)
    for col in ("i", "l"):
        assert expr_program(parse_expression("timeconvert(%s,'DAYS','SECONDS')" % col), TYPES) == _chain(col, ("mult", 86400))


# ------------------------------------------------------------------------------------------------ the limits
def test_limits_with_the_new_nodes():
    worst = "datetimeconvert(ts,'7:NANOSECONDS:EPOCH','3:DAYS:EPOCH','5:MINUTES')"
    assert len(expr_program(parse_expression(worst), TYPES)) == 13
    assert len(expr_program(parse_expression("floor(sqrt(abs(%s)))" % worst), TYPES)) == 16  # the unary ops spend no depth
    with pytest.raises(ValueError) as e:
        parse_expression("ceil(floor(sqrt(abs(%s))))" % worst)
    assert "17 ops" in str(e.value)
    with pytest.raises(ValueError) as e:
        parse_expression("%s + d" % worst)  # 0.0 + bucket + d: 17
    assert "ops" in str(e.value)
    # depth: a - (b - (c - mod(d, e))) stands five deep, the unary ops in between change nothing
    with pytest.raises(ValueError) as e:
        parse_expression("a - (b - (c - abs(mod(d, 3))))")
    assert "stack of 5" in str(e.value)
    parse_expression("a - (b - abs(mod(c, 3)))")
    with pytest.raises(ValueError) as e:
        parse_expression("ADD(mod(a, b), mod(c, 2), timeconvert(d,'DAYS','HOURS'), floor(e))")
    assert "5 columns" in str(e.value)


# ------------------------------------------------------------------------------------------------ WHERE literals
def test_long_literals_of_a_where_leaf():
    assert long_literal_text("1388534400", "x") == "1388534400" and long_literal_text("-5", "x") == "-5"
    assert long_literal_text("007", "x") == "7" and long_literal_text("+9223372036854775807", "x") == "9223372036854775807"
    assert long_literal_text("-9223372036854775808", "x") == "-9223372036854775808"
    for bad in ("1.5", "1.0", "1e3", "9223372036854775808", "-9223372036854775809", "abc", "", "0x10"):
        with pytest.raises(ValueError):
            long_literal_text(bad, "x")
    tc = "timeconvert(ts,'DAYS','SECONDS')"

    def where(cond):
        return parse_query("SELECT COUNT(*) FROM t WHERE " + cond, filter_expressions=True)
    assert where(tc + " = 86400").filter.predicate.values == ["86400"]
    assert where(tc + " IN (86400, 0172800)").filter.predicate.values == ["86400", "172800"]
    assert where(tc + " NOT IN (-86400)").filter.predicate.values == ["-86400"]
    assert where(tc + " BETWEEN 0 AND 86400").filter.predicate.values == ["0", "86400"]
    assert where(tc + " >= 5").filter.predicate.values == ["5", "*"]
    for cond in (tc + " = 1.5", tc + " IN (1, 2.0)", tc + " BETWEEN 0 AND 1e3", tc + " > 9223372036854775808",
                 "datetimeconvert(ts,'1:DAYS:EPOCH','1:HOURS:EPOCH','1:HOURS') = 0.5"):
        with pytest.raises(ValueError) as e:
            where(cond)
        assert "LONG literal" in str(e.value)
    # DOUBLE-typed leaves keep their decimal literals
    assert where("DIV(%s,1) = 86400.5" % tc).filter.predicate.values == ["86400.5"]
    assert where("floor(d) = 2.5").filter.predicate.values == ["2.5"]
    assert where("mod(l, 2) = 0").filter.predicate.column == "mod(l,2.0)"


# ------------------------------------------------------------------------------------------------ expr_compile
def _run_case_check(lines):
    check = build.build_case_check()
    res = subprocess.run([check], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout.split("\n")


def _lit(v):
    return ["l %016x" % (T.bits(v) & 0xffffffffffffffff)]


C0, C1, GT = ["c 0"], ["c 1"], ["o %d" % L.EXPR_GT]
O = {n: ["o %d" % getattr(L, "EXPR_" + n)] for n in ("ADD", "MULT", "DIV", "ABS", "CEIL", "FLOOR", "SQRT", "MOD", "LDIV", "SELECT")}
BAD_DIVISOR, BAD_DIVIDEND, BAD_MATH_TYPE = 10, 11, 12


@pytest.mark.parametrize("name, prog, code, word", [
    ("divisor_is_a_column", C0 + C1 + O["LDIV"], BAD_DIVISOR, "LITERAL right before it"),
    ("divisor_is_zero", C0 + _lit(0.0) + O["LDIV"], BAD_DIVISOR, "positive integer"),
    ("divisor_is_negative", C0 + _lit(-7.0) + O["LDIV"], BAD_DIVISOR, "positive integer"),
    ("divisor_is_a_half", C0 + _lit(2.5) + O["LDIV"], BAD_DIVISOR, "positive integer"),
    ("divisor_is_past_2_53", C0 + _lit(2.0 ** 53 + 2) + O["LDIV"], BAD_DIVISOR, "2^53"),
    ("divisor_is_nan", C0 + _lit(float("nan")) + O["LDIV"], BAD_DIVISOR, "positive integer"),
    ("divisor_is_a_computed_integer", C0 + _lit(3.0) + _lit(4.0) + O["MULT"] + O["LDIV"], BAD_DIVISOR, "LITERAL right before it"),
    ("dividend_is_a_sum", C0 + C1 + O["ADD"] + _lit(7.0) + O["LDIV"], BAD_DIVIDEND, "integral"),
    ("dividend_is_a_quotient", C0 + _lit(2.0) + O["DIV"] + _lit(7.0) + O["LDIV"], BAD_DIVIDEND, "integral"),
    ("dividend_is_a_floor", C0 + O["FLOOR"] + _lit(7.0) + O["LDIV"], BAD_DIVIDEND, "integral"),
    ("dividend_is_a_literal", C0 + O["ABS"] + _lit(9.0) + _lit(7.0) + O["LDIV"] + O["ADD"], BAD_DIVIDEND, "integral"),
    ("dividend_is_a_product_by_a_half", C0 + _lit(2.5) + O["MULT"] + _lit(7.0) + O["LDIV"], BAD_DIVIDEND, "integral"),
    ("dividend_is_a_product_with_the_literal_below", _lit(3.0) + C0 + O["MULT"] + _lit(7.0) + O["LDIV"], BAD_DIVIDEND, "integral"),
    ("dividend_is_a_modulus", C0 + _lit(9.0) + O["MOD"] + _lit(7.0) + O["LDIV"], BAD_DIVIDEND, "integral"),
    ("abs_of_a_boolean", C0 + C1 + GT + O["ABS"], BAD_MATH_TYPE, "not booleans"),
    ("floor_of_a_boolean", C0 + C1 + GT + O["FLOOR"], BAD_MATH_TYPE, "not booleans"),
    ("sqrt_of_a_boolean", C0 + C0 + C0 + C1 + GT + O["SQRT"] + O["SELECT"], BAD_MATH_TYPE, "not booleans"),
    ("mod_of_a_boolean", C0 + C0 + C1 + GT + O["MOD"], BAD_MATH_TYPE, "not booleans"),
    ("ldiv_of_a_boolean", C0 + C1 + GT + _lit(7.0) + O["LDIV"], BAD_MATH_TYPE, "not booleans"),
    ("unary_underflow", O["ABS"], 3, "underflow"),
    ("mod_underflow", C0 + O["MOD"], 3, "underflow"),
    ("ldiv_underflow", _lit(7.0) + O["LDIV"], 3, "underflow"),
])
def test_expr_compile_refuses(name, prog, code, word):
    got = _run_case_check(["prog %d" % len(prog)] + prog + ["rows 0"])
    assert got[0].startswith("error %d " % code) and word in got[0], got[0]


def test_expr_compile_accepts_the_chains_and_knows_the_unary_depth():
    # col * n / m / k, a product of a quotient, 2^53 itself as a divisor
    for prog in (C0 + _lit(300000.0) + O["MULT"] + _lit(3600000.0) + O["LDIV"] + _lit(3.0) + O["LDIV"],
                 C0 + _lit(900000.0) + O["LDIV"] + _lit(900000.0) + O["MULT"] + _lit(7.0) + O["LDIV"],
                 C0 + _lit(2.0 ** 53) + O["LDIV"], C0 + _lit(1.0) + O["LDIV"]):
        assert _run_case_check(["prog %d" % len(prog)] + prog + ["rows 0"])[0] == "ok 1 0"
    # a unary op leaves the depth: four values, each under three unary ops, is still a stack of 4 (16 ops)
    prog = (C0 + O["ABS"] + O["SQRT"] + O["FLOOR"]) + (C1 + O["CEIL"]) + ["c 2", "c 3"] + O["MOD"] + O["ADD"] + O["ADD"] + O["ABS"] * 3
    assert len(prog) == 14
    assert _run_case_check(["prog %d" % len(prog)] + prog + ["rows 0"])[0] == "ok 4 0"
    # the compared columns: a column under a unary op no longer reaches the comparison as it is, its neighbour does
    prog = ["c 5"] + ["c 6"] + C0 + O["FLOOR"] + C1 + GT + O["SELECT"]
    assert _run_case_check(["prog %d" % len(prog)] + prog + ["rows 0"])[0] == "ok 4 %d" % (1 << 3)


def test_the_ops_against_libm_and_int64_division_under_the_sanitizers():
    check = build.build_math_check()
    res = subprocess.run([check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    lines = res.stdout.split("\n")
    assert lines[0].startswith("ok edges ") and lines[1].startswith("ok ldiv ") and lines[2].startswith("ok programs ")
    assert int(lines[1].split()[2]) > 1000000 and int(lines[2].split()[2]) >= 1000


# ------------------------------------------------------------------------------------------------ the known answers
def test_the_references_vectors_through_the_emitted_programs():
    kat = T.load_kat()
    assert len(kat["datetimeconvert"]) == 6
    for case in kat["datetimeconvert"]:
        tree = parse_expression("dateTimeConvert(ts,'%s','%s','%s')" % (case["in"], case["out"], case["granularity"]))
        ops = expr_program(tree, TYPES)
        got = [T.run_program(ops, {"ts": v}) for v in case["input"]]
        assert got == [float(v) for v in case["expected"]], case["name"]
        assert all(T.bits(g) == T.bits(float(v)) for g, v in zip(got, case["expected"]))
    for case in kat["timeconvert"]:
        tree = parse_expression("timeConvert(DaysSinceEpoch,'%s','%s')" % (case["in"], case["out"]))
        ops = expr_program(tree, TYPES)
        assert [T.run_program(ops, {"DaysSinceEpoch": v}) for v in case["input"]] == [float(v) for v in case["expected"]]
        assert case["expected"] == [v * 86400 for v in case["input"]]


def test_truncation_is_toward_zero_in_the_interpreter_too():
    ops = expr_program(parse_expression("timeconvert(ts,'MILLISECONDS','DAYS')"), TYPES)
    assert [T.bits(T.run_program(ops, {"ts": v})) for v in (-1, -86399999, -86400000, -86400001, 86399999, 86400000)] == \
        [T.bits(x) for x in (0.0, 0.0, -1.0, -1.0, 0.0, 1.0)]
