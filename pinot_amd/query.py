"""Query model of the path: the subset of Pinot's QueryContext that reaches the per-segment group-by operator.

Mirrors (names and meaning):
  Predicate / FilterContext   pinot-core .../query/request/context/predicate/*, FilterContext (AND / OR /
                              PREDICATE; NOT is accepted too)
  QueryContext                core/query/request/context/QueryContext.java:164-317 (filter, group-by
                              expressions, aggregation functions, numGroupsLimit)
A small parser for the SQL/PQL subset the reference tests use (comparisons, BETWEEN, IN / NOT IN, AND / OR /
NOT, GROUP BY, TOP / LIMIT / ORDER BY accepted and ignored: trimming and ordering are broker-side) turns
strings such as the README AdAnalytics query into a QueryContext.  Literals stay strings: they are converted
per column type by the dictionary lookup, exactly as PredicateUtils.getStoredValue does.
"""
import ctypes
import re
import time

import decimal

from . import _lib as L

EQ, NOT_EQ, IN, NOT_IN, RANGE = "EQ", "NOT_EQ", "IN", "NOT_IN", "RANGE"
REGEXP_LIKE = "REGEXP_LIKE"  # RegexpLikePredicate; col LIKE 'p' is one too, after like_to_regexp_like
UNBOUNDED = "*"  # RangePredicate.UNBOUNDED
_PRED_CODE = {EQ: L.PRED_EQ, NOT_EQ: L.PRED_NOT_EQ, IN: L.PRED_IN, NOT_IN: L.PRED_NOT_IN, RANGE: L.PRED_RANGE,
              REGEXP_LIKE: L.PRED_REGEXP_LIKE}
AGG_FUNCTIONS = {"COUNT": L.AGG_COUNT, "SUM": L.AGG_SUM, "MIN": L.AGG_MIN, "MAX": L.AGG_MAX, "AVG": L.AGG_AVG,
                 "DISTINCTCOUNT": L.AGG_DISTINCTCOUNT}
DEFAULT_NUM_GROUPS_LIMIT = 100000  # InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT (:70)
DEFAULT_LIMIT = 10  # QueryContext default LIMIT / TOP
DEFAULT_MIN_SERVER_GROUP_TRIM_SIZE = 5000  # InstancePlanMakerImplV2.DEFAULT_MIN_SERVER_GROUP_TRIM_SIZE
DEFAULT_GROUP_TRIM_THRESHOLD = 1000000  # InstancePlanMakerImplV2.DEFAULT_GROUPBY_TRIM_THRESHOLD


PERCENTILE_MAX_E4 = 1000000  # PGPU_AGG_PERCENTILE_MAX_E4: the percentile in ten-thousandths, at most 100
_PERCENTILE_OTHERS = ("EST", "TDIGEST", "RAWEST", "RAWTDIGEST", "MV", "ESTMV", "TDIGESTMV", "RAWESTMV", "RAWTDIGESTMV")


def percentile_code(percentile):
    """A percentile (number or decimal string, 0 .. 100, a multiple of 0.0001) in ten-thousandths; ValueError
    otherwise.  p_e4 / 10000.0 is the double of the decimal literal, which is what Pinot's arithmetic uses."""
    try:
        d = decimal.Decimal(percentile if isinstance(percentile, (str, int)) else repr(percentile))
    except (decimal.InvalidOperation, TypeError, ValueError):
        raise ValueError("PERCENTILE: %r is not a percentile" % (percentile,))
    if not d.is_finite() or d < 0 or d > 100:
        raise ValueError("PERCENTILE: percentile %s outside [0, 100]" % (percentile,))
    e4 = d * 10000
    if e4 != e4.to_integral_value():
        raise ValueError("PERCENTILE: percentile %s is not a multiple of 0.0001" % (percentile,))
    return int(e4)


def percentile_name(p_e4):
    """The canonical name of the exact percentile: PERCENTILE95, PERCENTILE99.9 (a whole one without a fraction)."""
    whole, frac = divmod(p_e4, 10000)
    return "PERCENTILE%d" % whole + (".%04d" % frac).rstrip("0") * (frac != 0)


def percentile_e4(name):
    """The percentile of a canonical function name in ten-thousandths, None for every other function."""
    if not name.startswith("PERCENTILE"):
        return None
    return percentile_code(name[len("PERCENTILE"):])


def function_name(fn, percentile=None):
    """An aggregation function's canonical name: upper case, underscores dropped (DISTINCT_COUNT = DISTINCTCOUNT), as
    AggregationFunctionType.getAggregationFunctionType normalises it.  The exact percentile carries its percentile in
    the name: PERCENTILE95(x), PERCENTILE(x, 95) and PERCENTILE(x, '95.0') are all PERCENTILE95.  The estimating and
    multi-value percentile functions are not supported (ValueError)."""
    name = fn.upper().replace("_", "")
    if not name.startswith("PERCENTILE"):
        if percentile is not None:
            raise ValueError("%s takes one argument" % name)
        return name
    suffix = name[len("PERCENTILE"):]
    for other in _PERCENTILE_OTHERS:
        if suffix.startswith(other):
            raise ValueError("unsupported aggregation function PERCENTILE%s: only the exact single-value PERCENTILE "
                             "runs on the GPU path" % other)
    if (suffix == "") == (percentile is None):
        raise ValueError("PERCENTILE takes its percentile in the name (PERCENTILE95(x)) or as the second argument "
                         "(PERCENTILE(x, 95)), got %s" % fn)
    return percentile_name(percentile_code(suffix if percentile is None else percentile))


# ================================================================================ expressions inside aggregations
# SUM(price * qty): the reference's arithmetic transform functions (AdditionTransformFunction & co).  A tree is
# ("col", name), ("lit", text) or (fn, [args]) with fn in add / sub / mult / div; infix operators are binary nodes.
_EXPR_FUNCTIONS = {"ADD": "add", "PLUS": "add", "SUB": "sub", "MINUS": "sub", "MULT": "mult", "TIMES": "mult",
                   "DIV": "div", "DIVIDE": "div"}
_EXPR_OPCODE = {"add": L.EXPR_ADD, "sub": L.EXPR_SUB, "mult": L.EXPR_MULT, "div": L.EXPR_DIV}
_EXPR_CHARS = re.compile(r"[()+\-*/]")
_CASE_START = re.compile(r"\s*case\s+when\s", re.I)


def is_expression(column):
    """An aggregation's argument that is no plain column name (and not COUNT's *)."""
    return isinstance(column, str) and column != "*" and \
        (_EXPR_CHARS.search(column) is not None or _CASE_START.match(column) is not None)


# Conditional expressions (CASE WHEN clicks > 100 THEN 1 ELSE 0 END): the reference's CaseTransformFunction,
# BinaryOperatorTransformFunction, And / OrOperatorTransformFunction and LiteralTransformFunction.  Nodes: a comparison
# (equals(a,b) ..), ("and" / "or", [conditions]) and ("case", [when1..whenN, then1..thenN, else]) -- the reference's
# argument order.  A literal that is a direct operand of a comparison or a THEN / ELSE is ("lit", its typed text): what
# the server sees, Long.toString of an integer literal and Double.toString of a decimal one.
_CMP_FUNCTIONS = {"EQUALS": "equals", "NOT_EQUALS": "not_equals", "GREATER_THAN": "greater_than",
                  "GREATER_THAN_OR_EQUAL": "greater_than_or_equal", "LESS_THAN": "less_than",
                  "LESS_THAN_OR_EQUAL": "less_than_or_equal"}
_CMP_SQL = {"=": "equals", "!=": "not_equals", "<>": "not_equals", ">": "greater_than", ">=": "greater_than_or_equal",
            "<": "less_than", "<=": "less_than_or_equal"}
_CMP_OPCODE = {"equals": L.EXPR_EQ, "not_equals": L.EXPR_NE, "greater_than": L.EXPR_GT,
               "greater_than_or_equal": L.EXPR_GE, "less_than": L.EXPR_LT, "less_than_or_equal": L.EXPR_LE}
_CMP_NOT = {"equals": "not_equals", "not_equals": "equals", "greater_than": "less_than_or_equal",
            "less_than_or_equal": "greater_than", "less_than": "greater_than_or_equal",
            "greater_than_or_equal": "less_than"}
_BOOL_NODES = tuple(_CMP_OPCODE) + ("and", "or")
INT, LONG, FLOAT, DOUBLE = "INT", "LONG", "FLOAT", "DOUBLE"  # the types of section "typing" below; BOOLEAN beside them
BOOLEAN = "BOOLEAN"


# Math and time functions (SingleParamMathTransformFunction, ModuloTransformFunction, TimeConversionTransformFunction,
# DateTimeConversionTransformFunction epoch to epoch).  Nodes: ("abs" | "ceil" | "floor" | "sqrt", [x]), ("mod", [a, b]),
# ("timeconvert", [col, ("str", in unit), ("str", out unit)]) and ("datetimeconvert", [col, ("str", in format),
# ("str", out format), ("str", granularity)]); a ("str", text) leaf is a string argument as it was written.
_MATH_FUNCTIONS = {"ABS": "abs", "CEIL": "ceil", "FLOOR": "floor", "SQRT": "sqrt"}
_MATH_OPCODE = {"abs": L.EXPR_ABS, "ceil": L.EXPR_CEIL, "floor": L.EXPR_FLOOR, "sqrt": L.EXPR_SQRT}
_TIME_FUNCTIONS = {"TIMECONVERT": "timeconvert", "DATETIMECONVERT": "datetimeconvert"}
_DECLINED_FUNCTIONS = {"EXP": "Math.exp", "LN": "Math.log"}
_LEAVES = ("col", "lit", "str")
# java.util.concurrent.TimeUnit in nanoseconds; WEEKS is CustomTimeUnitTransformer's / DateTimeTransformUnit's, an output
# unit only: the milliseconds divided by 604800000
_UNIT_NANOS = {"NANOSECONDS": 1, "MICROSECONDS": 1000, "MILLISECONDS": 10 ** 6, "SECONDS": 10 ** 9,
               "MINUTES": 60 * 10 ** 9, "HOURS": 3600 * 10 ** 9, "DAYS": 86400 * 10 ** 9}
_WEEK_MILLIS = 604800000
_CALENDAR_UNITS = ("WEEKS", "MONTHS", "YEARS")
_EXACT = 2 ** 53


def transform_function_name(fn):
    """The canonical key of a transform function's name: upper case, underscores dropped (TIME_CONVERT is TIMECONVERT),
    as the reference's TransformFunctionFactory normalises it -- for the math and time functions only; the arithmetic and
    comparison names keep their underscores (NOT_EQUALS)."""
    up = fn.upper().replace("_", "")
    return up if up in _MATH_FUNCTIONS or up in _TIME_FUNCTIONS or up in _DECLINED_FUNCTIONS or up == "MOD" else fn.upper()


def _positive_int(text, what):
    if not re.fullmatch(r"\d+", text) or int(text) < 1:
        raise ValueError("%s: size %r is not a positive integer" % (what, text))
    return int(text)


def _epoch_format(text, what, output):
    """(size, unit) of 'n:UNIT:EPOCH'."""
    parts = text.split(":")
    if len(parts) >= 3 and parts[2].upper() == "SIMPLE_DATE_FORMAT":
        raise ValueError("%s: SIMPLE_DATE_FORMAT in %r: its values are strings, only EPOCH formats are supported" % (what, text))
    if len(parts) != 3 or parts[2].upper() != "EPOCH":
        raise ValueError("%s: %r is no format 'size:UNIT:EPOCH'" % (what, text))
    size, unit = _positive_int(parts[0], what), parts[1].upper()
    _check_unit(unit, what, output)
    return size, unit


def _check_unit(unit, what, output):
    if unit in _CALENDAR_UNITS and not (output and unit == "WEEKS"):
        raise ValueError("%s: %s as the %s unit is not supported (%s)" % (
            what, unit, "output" if output else "input",
            "MONTHS and YEARS need the calendar" if output else "WEEKS, MONTHS and YEARS are output units only"))
    if unit not in _UNIT_NANOS and unit != "WEEKS":
        raise ValueError("%s: unknown time unit %r (NANOSECONDS .. DAYS%s)" % (what, unit, ", WEEKS" if output else ""))


def _to_millis(unit):
    """TimeUnit.toMillis as a chain step."""
    nanos = _UNIT_NANOS[unit]
    return ("mult", nanos // 10 ** 6) if nanos >= 10 ** 6 else ("ldiv", 10 ** 6 // nanos)


def _from_millis(unit):
    """TimeUnit.convert(ms, MILLISECONDS) / DateTimeTransformUnit.fromMillis as a chain step."""
    if unit == "WEEKS":
        return ("ldiv", _WEEK_MILLIS)
    nanos = _UNIT_NANOS[unit]
    return ("ldiv", nanos // 10 ** 6) if nanos >= 10 ** 6 else ("mult", 10 ** 6 // nanos)


def time_chain(tree):
    """The long arithmetic of a time node over its column as [("mult" | "ldiv", n)], n a positive integer: what the
    program does after pushing the column (x, LITERAL n, MULT / LDIV each).  Steps by 1 are dropped and adjacent
    multiplications folded into one constant; divisions stay apart, so the same arguments always give the same program.
    timeconvert is TimeUnit.convert -- one multiplication where the output unit is finer, one truncating division where
    it is coarser -- or, to WEEKS, toMillis and / 604800000 (CustomTimeUnitTransformer).  datetimeconvert is
    EpochToEpochTransformer's order: x * n, toMillis, / G * G with G the granularity in milliseconds, fromMillis, / m."""
    what = tree[0].upper()
    if tree[0] == "timeconvert":
        unit_in, unit_out = tree[1][1][1].upper(), tree[1][2][1].upper()
        _check_unit(unit_in, what, False)
        _check_unit(unit_out, what, True)
        if unit_out == "WEEKS":
            steps = [_to_millis(unit_in), ("ldiv", _WEEK_MILLIS)]
        else:
            a, b = _UNIT_NANOS[unit_in], _UNIT_NANOS[unit_out]
            steps = [("mult", a // b)] if a >= b else [("ldiv", b // a)]
    else:
        n, unit_in = _epoch_format(tree[1][1][1], what, False)
        m, unit_out = _epoch_format(tree[1][2][1], what, True)
        gran = tree[1][3][1].split(":")
        if len(gran) != 2:
            raise ValueError("%s: %r is no granularity 'size:UNIT'" % (what, tree[1][3][1]))
        gsize, gunit = _positive_int(gran[0], what), gran[1].upper()
        if gunit not in _UNIT_NANOS:
            raise ValueError("%s: unknown granularity unit %r (NANOSECONDS .. DAYS)" % (what, gunit))
        # DateTimeGranularitySpec.granularityToMillis: TimeUnit.MILLISECONDS.convert(size, unit), truncating
        g = gsize * _UNIT_NANOS[gunit] // 10 ** 6
        if g < 1:
            raise ValueError("%s: granularity %s is below one millisecond (the reference divides by zero)" % (what, tree[1][3][1]))
        steps = [("mult", n), _to_millis(unit_in), ("ldiv", g), ("mult", g), _from_millis(unit_out), ("ldiv", m)]
    out = []
    for kind, k in steps:
        if k == 1:
            continue
        if kind == "mult" and out and out[-1][0] == "mult":
            out[-1] = ("mult", out[-1][1] * k)
        else:
            out.append((kind, k))
    for kind, k in out:
        if k > _EXACT:
            raise ValueError("%s: the constant %d is beyond 2^53" % (what, k))
    return out


def math_node(name, args):
    """abs / ceil / floor / sqrt of one number that is no literal; mod of two numbers (either may be a literal)."""
    if name == "mod":
        if len(args) != 2:
            raise ValueError("MOD takes exactly 2 arguments, got %d" % len(args))
        return ("mod", [_number(a, "MOD") for a in args])
    if len(args) != 1:
        raise ValueError("%s takes exactly 1 argument, got %d" % (name.upper(), len(args)))
    if args[0][0] == "lit":
        raise ValueError("%s of the literal %s: its argument is a column or an expression" % (name.upper(), args[0][1]))
    return (name, [_number(args[0], name.upper())])


def time_node(name, args):
    """timeconvert(col, 'IN', 'OUT') / datetimeconvert(col, 'n:UNIT:EPOCH', 'm:UNIT:EPOCH', 'g:UNIT') over a column (INT
    or LONG: expr_program checks where it knows the types); every other shape is declined by name."""
    want = 3 if name == "timeconvert" else 4
    if len(args) != want:
        raise ValueError("%s takes exactly %d arguments, got %d" % (name.upper(), want, len(args)))
    if args[0][0] != "col":
        raise ValueError("%s over %s: its first argument is an INT or LONG column (the reference casts a nested "
                         "function's value to long, and there is no cast)" % (name.upper(), expr_name(args[0])))
    for a in args[1:]:
        if a[0] != "str":
            raise ValueError("%s: argument %s is no string literal" % (name.upper(), expr_name(a)))
    tree = (name, list(args))
    time_chain(tree)  # (declines what it cannot lower)
    return tree


class _Lit(str):
    """A literal's name in arithmetic (the double's shortest form, as before) that remembers the text it was read
    from: a comparison or a CASE branch types its literal operands by that text (0 is not 0.0)."""
    raw = None


def java_double_text(d):
    """Double.toString(d) for a finite double of at most 15 significant digits (ValueError beyond: older JDKs do not
    always print the shortest digits there): plain notation with at least one digit after the point for
    1e-3 <= |d| < 1e7, d.dddE[-]n otherwise."""
    if d != d or d in (float("inf"), float("-inf")):
        raise ValueError("literal %r is not a finite number" % (d,))
    sign, digits, exp = decimal.Decimal(repr(d)).as_tuple()
    digits = list(digits)
    while len(digits) > 1 and digits[-1] == 0:  # 1e22's repr is exact digits and zeros
        digits.pop()
        exp += 1
    neg = "-" if repr(d).startswith("-") else ""
    if d == 0:
        return neg + "0.0"
    if len(digits) > 15:
        raise ValueError("literal %r has more than 15 significant digits: its text on the server is not certain" % (d,))
    s = "".join(map(str, digits))
    point = len(s) + exp  # the value is 0.s * 10^point
    if 1e-3 <= abs(d) < 1e7:
        if point <= 0:
            return neg + "0." + "0" * -point + s
        whole, frac = (s + "0" * (point - len(s)))[:point], s[point:]
        return neg + whole + "." + (frac or "0")
    return neg + s[0] + "." + (s[1:] or "0") + "E%d" % (point - 1)


def typed_literal_text(raw):
    """The text of a literal as the server sees it (RequestContextUtils.getExpression): Long.toString of an integer
    literal, Double.toString of a decimal one.  ValueError for anything that is no number (strings, true / false)."""
    raw = str(raw).strip()
    if re.fullmatch(r"[+-]?\d+", raw):
        return str(int(raw))
    if not re.fullmatch(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", raw):
        raise ValueError("%r is not a numeric literal (strings, timestamps and true / false are not supported in a "
                         "comparison or a CASE branch)" % (raw,))
    return java_double_text(float(raw))


def literal_type(text):
    """NumberUtils.createNumber (commons-lang3 3.5) of a typed literal text, as LiteralTransformFunction types it: an
    integer is INT where it fits int32, else LONG where it fits int64; a decimal with at most 7 digits between the
    point and the E (or the end) whose float is finite and not zero-from-nonzero is FLOAT, else with at most 16 DOUBLE.
    Everything else (BigInteger, BigDecimal) is declined."""
    if re.fullmatch(r"-?\d+", text):
        v = int(text)
        if -2 ** 31 <= v < 2 ** 31:
            return INT
        if -2 ** 63 <= v < 2 ** 63:
            return LONG
        raise ValueError("integer literal %s does not fit a LONG" % text)
    m = re.fullmatch(r"-?\d+\.(\d+)(E-?\d+)?", text)
    if not m:
        raise ValueError("%r is no typed literal text" % (text,))
    d, ndec = float(text), len(m.group(1))
    if ndec <= 7:
        f = _f32(d)
        if f == f and abs(f) != float("inf") and not (f == 0.0 and d != 0.0):
            return FLOAT
    if ndec <= 16:
        return DOUBLE
    raise ValueError("literal %s is a BigDecimal on the server" % text)


def _f32(d):
    """(double)(float)d."""
    try:
        return ctypes.c_float(d).value
    except OverflowError:
        return float("inf") if d > 0 else float("-inf")


def _typed(arg):
    """A comparison's or a CASE branch's direct operand: a literal becomes its typed text."""
    if arg[0] == "col" and arg[1].lower() in ("true", "false", "null"):
        raise ValueError("%s in a comparison or a CASE branch: boolean and NULL literals are not supported" % arg[1])
    if arg[0] != "lit":
        return arg
    text = typed_literal_text(getattr(arg[1], "raw", None) or arg[1])
    literal_type(text)  # (declines what has no type)
    return ("lit", text)


def _is_bool(tree):
    return tree[0] in _BOOL_NODES


def _number(tree, where):
    if _is_bool(tree):
        raise ValueError("boolean %s used as a number in %s: a condition stands after WHEN only" % (expr_name(tree), where))
    return tree


def cmp_node(fn, a, b):
    """The comparison node `fn` (a canonical name) over two numbers; a literal-only condition is declined."""
    a, b = _typed(_number(a, fn)), _typed(_number(b, fn))
    if not expr_columns(a) and not expr_columns(b):
        raise ValueError("literal-only condition %s(%s,%s): a condition needs a column operand" % (fn, a[1], b[1]))
    return (fn, [a, b])


def logic_node(fn, args):
    """and(..) / or(..) over conditions (the reference's n-ary form)."""
    if len(args) < 2:
        raise ValueError("%s takes at least 2 arguments, got %d" % (fn.upper(), len(args)))
    for a in args:
        if not _is_bool(a):
            raise ValueError("%s of %s: AND / OR join conditions" % (fn.upper(), expr_name(a)))
    return (fn, list(args))


def case_node(whens, thens, els):
    """case(when1..whenN, then1..thenN, else).  A missing ELSE is declined: the reference's NULL there makes the
    result a STRING."""
    if els is None:
        raise ValueError("CASE without ELSE: the reference's result type is then STRING, which no aggregation here reads")
    if not whens or len(whens) != len(thens):
        raise ValueError("CASE takes as many THENs as WHENs, and at least one")
    for w in whens:
        if not _is_bool(w):
            raise ValueError("CASE WHEN %s: a WHEN takes a condition (a comparison, AND, OR)" % expr_name(w))
    return ("case", list(whens) + [_typed(_number(t, "a THEN")) for t in thens] + [_typed(_number(els, "an ELSE"))])


def case_parts(tree):
    """(whens, thens, else) of a case node."""
    n = (len(tree[1]) - 1) // 2
    return tree[1][:n], tree[1][n:2 * n], tree[1][2 * n]


def expr_node(fn, args):
    """The node of function `fn` (a name or SQL alias, any case) over `args`, its argument count checked."""
    up = fn.upper()
    if up in _CMP_FUNCTIONS:
        if len(args) != 2:
            raise ValueError("%s takes exactly 2 arguments, got %d" % (up, len(args)))
        return cmp_node(_CMP_FUNCTIONS[up], args[0], args[1])
    if up in ("AND", "OR"):
        return logic_node(up.lower(), args)
    if up == "CASE":
        if len(args) % 2 == 0:
            raise ValueError("case(when.., then.., else) takes an odd number of arguments (a missing ELSE is not "
                             "supported), got %d" % len(args))
        n = (len(args) - 1) // 2
        return case_node(args[:n], args[n:2 * n], args[2 * n])
    key = transform_function_name(fn)
    if key in _DECLINED_FUNCTIONS:
        raise ValueError("%s is not supported: Java's %s is not correctly rounded, so its bits cannot be promised"
                         % (key, _DECLINED_FUNCTIONS[key]))
    if key in _MATH_FUNCTIONS or key == "MOD":
        return math_node(_MATH_FUNCTIONS.get(key, "mod"), args)
    if key in _TIME_FUNCTIONS:
        return time_node(_TIME_FUNCTIONS[key], args)
    for a in args:
        if a[0] == "str":
            raise ValueError("string literal '%s' as an argument of %s" % (a[1], fn))
    name = _EXPR_FUNCTIONS.get(up)
    if name is None:
        raise ValueError("unknown function %s in an aggregation's argument (ADD, SUB, MULT, DIV and their aliases "
                         "PLUS, MINUS, TIMES, DIVIDE, the comparison functions, AND, OR, CASE, ABS, CEIL, FLOOR, SQRT, MOD, "
                         "TIMECONVERT and DATETIMECONVERT are supported)" % fn)
    if name in ("sub", "div") and len(args) != 2:
        raise ValueError("%s takes exactly 2 arguments, got %d" % (name.upper(), len(args)))
    if len(args) < 2:
        raise ValueError("%s takes at least 2 arguments, got %d" % (name.upper(), len(args)))
    return (name, [_number(a, name.upper()) for a in args])


def expr_literal(text):
    """A numeric literal node: Double.parseDouble of its text, named by the double's shortest form."""
    try:
        name = _Lit(repr(float(text)))
    except ValueError:
        raise ValueError("%r is not a numeric literal" % (text,))
    name.raw = str(text)
    return ("lit", name)


def expr_columns(tree):
    """The distinct columns of a tree, in first-use order."""
    out = []

    def walk(t):
        if t[0] == "col":
            if t[1] not in out:
                out.append(t[1])
        elif t[0] not in _LEAVES:
            for a in t[1]:
                walk(a)
    walk(tree)
    return out


def has_conditional(tree):
    """Whether a tree holds a comparison, AND / OR or a CASE: its program then depends on the columns' types."""
    return tree[0] not in _LEAVES and (tree[0] in _BOOL_NODES + ("case",) or any(has_conditional(a) for a in tree[1]))


def _widen(a, b):
    """calculateResultMetadata's fold of two branch types."""
    if a == b:
        return a
    if {a, b} == {INT, LONG}:
        return LONG
    return DOUBLE


def expr_type(tree, types):
    """The reference's data type of a numeric tree: a column's, a typed literal's, DOUBLE of an arithmetic node, R of a
    CASE (folded over ELSE, then the THENs in order).  types: column name -> 'INT' | 'LONG' | 'FLOAT' | 'DOUBLE' |
    'STRING'.  STRING operands are declined."""
    if tree[0] == "col":
        t = types[tree[1]]
        t = L.TYPE_NAME_OF.get(t, t) if not isinstance(t, str) else t
        if t not in (INT, LONG, FLOAT, DOUBLE):
            raise ValueError("expression over %s column %s" % (t, tree[1]))
        return t
    if tree[0] == "lit":
        return literal_type(tree[1])
    if tree[0] == "case":
        _, thens, els = case_parts(tree)
        r = expr_type(els, types)
        for t in thens:
            r = _widen(r, expr_type(t, types))
        return r
    if _is_bool(tree):
        return BOOLEAN
    if tree[0] in ("timeconvert", "datetimeconvert"):
        return LONG
    return DOUBLE


class _AnyDouble(dict):
    """Column types for counting ops only (check_expr_limits): the count does not depend on them."""

    def __missing__(self, key):
        return DOUBLE


def expr_name(tree):
    """The expression in the reference's function form: mult(price,qty), add(div(a,b),2.5)."""
    if tree[0] in ("col", "lit"):
        return tree[1]
    if tree[0] == "str":  # (as the reference prints a string literal)
        return "'%s'" % tree[1]
    return "%s(%s)" % (tree[0], ",".join(expr_name(a) for a in tree[1]))


def _negated(cond):
    """The condition that holds exactly where `cond` does not.  Comparisons are Double.compare's total order, so the
    negation of a > b is a <= b for every pair of values, NaN included."""
    if cond[0] == "and":
        return ("or", [_negated(c) for c in cond[1]])
    if cond[0] == "or":
        return ("and", [_negated(c) for c in cond[1]])
    return (_CMP_NOT[cond[0]], cond[1])


def _literal_value(text, as_type):
    """The double the reference reads a typed literal as under `as_type`: its integer under INT / LONG, (double)(float)
    under FLOAT, its plain double under DOUBLE."""
    if as_type == FLOAT:
        return _f32(float(text))
    if as_type in (INT, LONG) and re.fullmatch(r"-?\d+", text):
        return float(int(text))
    return float(text)


def expr_program(tree, types=None):
    """The postfix program of a tree as (op, column name or None, literal) triples, all ops binary: ADD(x1..xn) is
    ((0.0 + the literal arguments in order) + v1) + v2 ... over the non-literal arguments in order, MULT likewise from
    1.0 (AdditionTransformFunction.java:44-82, MultiplicationTransformFunction.java:34-82); SUB and DIV are a op b.

    A tree with a comparison or a CASE needs `types` (column name -> 'INT' | 'LONG' | 'FLOAT' | 'DOUBLE' | 'STRING'):
    the value of a literal there depends on them.  A comparison is a, b, CMP with each literal read as its own type; a
    LONG side against a FLOAT or DOUBLE side is declined.  CASE WHEN c1 THEN r1 .. ELSE e END is e, rN, cN, SELECT, ..,
    r1, c1, SELECT with each THEN / ELSE literal read as the CASE's result type R.  A condition joined by AND / OR would
    stand as two booleans and two operands above ELSE and THEN, a stack of 5, so it is lowered to further SELECTs that
    choose the same branch for every doc: WHEN c1 OR c2 THEN r is WHEN c1 THEN r WHEN c2 THEN r, and WHEN c1 AND c2 THEN
    r ELSE e is WHEN not c1 THEN e WHEN not c2 THEN e ELSE r (_negated).  Every branch is evaluated for every doc
    anyway, so a branch emitted twice has the same bits both times."""
    ops = []
    if types is None and has_conditional(tree):
        raise ValueError("expression %s: the program of a comparison or a CASE depends on the column types "
                         "(expr_program(tree, types))" % expr_name(tree))

    def emit_cmp(c):
        a, b = c[1]
        ta, tb = expr_type(a, types), expr_type(b, types)
        for x, y in ((ta, tb), (tb, ta)):
            if x == LONG and y in (FLOAT, DOUBLE) and not isinstance(types, _AnyDouble):
                raise ValueError("%s compares a LONG with a %s: the reference's result there is a known bug that is "
                                 "not reproduced" % (expr_name(c), y))
        for x, t in ((a, ta), (b, tb)):
            if x[0] == "lit":
                ops.append((L.EXPR_LITERAL, None, _literal_value(x[1], t)))
            else:
                emit(x)
        ops.append((_CMP_OPCODE[c[0]], None, 0.0))

    def emit_select(cond, then, els):
        """cond ? then() : els(), the else emitted first."""
        if cond[0] == "or":
            rest = cond[1][1:]
            emit_select(cond[1][0], then, lambda: emit_select(rest[0] if len(rest) == 1 else ("or", rest), then, els))
        elif cond[0] == "and":
            rest = cond[1][1:]
            emit_select(_negated(cond[1][0]), els, lambda: emit_select(rest[0] if len(rest) == 1 else ("and", rest), then, els))
        else:
            els()
            then()
            emit_cmp(cond)
            ops.append((L.EXPR_SELECT, None, 0.0))

    def emit_case(t):
        whens, thens, els = case_parts(t)
        r = expr_type(t, types)

        def branch(x):
            if x[0] == "lit":
                return lambda: ops.append((L.EXPR_LITERAL, None, _literal_value(x[1], r)))
            return lambda: emit(x)

        def chain(k):
            if k == len(whens):
                return branch(els)
            return lambda: emit_select(whens[k], branch(thens[k]), chain(k + 1))
        chain(0)()

    def emit(t):
        if t[0] == "col":
            ops.append((L.EXPR_COLUMN, t[1], 0.0))
        elif t[0] == "lit":
            ops.append((L.EXPR_LITERAL, None, float(t[1])))
        elif t[0] == "case":
            emit_case(t)
        elif _is_bool(t):
            raise ValueError("boolean %s used as a number" % expr_name(t))
        elif t[0] in _MATH_OPCODE:
            emit(t[1][0])
            ops.append((_MATH_OPCODE[t[0]], None, 0.0))
        elif t[0] == "mod":
            emit(t[1][0])
            emit(t[1][1])
            ops.append((L.EXPR_MOD, None, 0.0))
        elif t[0] in ("timeconvert", "datetimeconvert"):
            col = t[1][0][1]
            if types is not None and not isinstance(types, _AnyDouble) and expr_type(t[1][0], types) not in (INT, LONG):
                raise ValueError("%s over %s column %s: its first argument is an INT or LONG column (the reference "
                                 "casts the value to long, and there is no cast)" % (t[0].upper(), expr_type(t[1][0], types), col))
            ops.append((L.EXPR_COLUMN, col, 0.0))
            for kind, k in time_chain(t):
                ops.append((L.EXPR_LITERAL, None, float(k)))
                ops.append((L.EXPR_MULT if kind == "mult" else L.EXPR_LDIV, None, 0.0))
        elif t[0] in ("sub", "div"):
            emit(t[1][0])
            emit(t[1][1])
            ops.append((_EXPR_OPCODE[t[0]], None, 0.0))
        else:
            acc = 0.0 if t[0] == "add" else 1.0
            for a in t[1]:
                if a[0] == "lit":
                    acc = acc + float(a[1]) if t[0] == "add" else acc * float(a[1])
            rest = [a for a in t[1] if a[0] != "lit"]
            # A CASE needs the whole stack.  As the first operand it is emitted before the folded literal: acc op v and
            # v op acc are the same double (IEEE addition and multiplication commute).
            first_below = has_conditional(rest[0])
            if first_below:
                emit(rest[0])
            ops.append((L.EXPR_LITERAL, None, acc))
            if first_below:
                ops.append((_EXPR_OPCODE[t[0]], None, 0.0))
            for a in rest[first_below:]:
                emit(a)
                ops.append((_EXPR_OPCODE[t[0]], None, 0.0))
    emit(tree)
    return ops


def check_expr_limits(tree):
    """ValueError where the tree's program is beyond what a virtual column holds (pgpu_table_add_expression: 16 ops, an
    evaluation stack of 4, 4 distinct columns).  Every ADD / MULT node spends one op and one stack level on its folded
    literal, so a long infix chain -- a + b + c + d + e nests four binary nodes -- is deeper than it looks: the n-ary
    form ADD(a, b, c, d, e) is one node."""
    ops = expr_program(tree, _AnyDouble())  # (the count does not depend on the column types)
    depth = most = 0
    for op, _, _ in ops:
        depth += 1 if op in (L.EXPR_COLUMN, L.EXPR_LITERAL) else -2 if op == L.EXPR_SELECT else \
            0 if L.EXPR_ABS <= op <= L.EXPR_SQRT else -1
        most = max(most, depth)
    name = expr_name(tree)
    hint = "; the n-ary forms ADD(x1, .., xn) / MULT(x1, .., xn) take one op per argument more and no nesting"
    if has_conditional(tree):
        hint += "; a CASE spends ELSE, THEN and the two operands of a comparison, and four ops per comparison"
    if len(ops) > L.EXPR_MAX_OPS:
        raise ValueError("expression %s compiles to %d ops, more than %d%s" % (name, len(ops), L.EXPR_MAX_OPS, hint))
    if most > L.EXPR_MAX_DEPTH:
        raise ValueError("expression %s needs an evaluation stack of %d, more than %d%s" % (name, most, L.EXPR_MAX_DEPTH, hint))
    if len(expr_columns(tree)) > L.EXPR_MAX_COLUMNS:
        raise ValueError("expression %s names %d columns, more than %d" % (name, len(expr_columns(tree)), L.EXPR_MAX_COLUMNS))


def long_literal_text(text, where):
    """Long.parseLong of a predicate's literal, as the reference's raw LONG predicate evaluators read it
    (EqualsPredicateEvaluatorFactory.java:63-64: a decimal or a value past int64 is its BadQueryRequestException), given
    back as the decimal text that is passed on.  Within +-2^53, where the plan keeps such an expression, comparing the
    doubles is comparing the longs."""
    text = str(text).strip()
    if not re.fullmatch(r"[+-]?\d+", text) or not -2 ** 63 <= int(text) < 2 ** 63:
        raise ValueError("%r is no LONG literal: %s is LONG-typed and compares with integers that fit int64" % (text, where))
    return str(int(text))


def long_predicate(p):
    """Predicate p, whose left-hand side is LONG-typed, with every literal read by long_literal_text."""
    vals = [v if (p.type == RANGE and v == UNBOUNDED) else long_literal_text(v, p.column) for v in p.values]
    return Predicate(p.type, p.column, vals, p.lower_inclusive, p.upper_inclusive)


def _check_expr(tree):
    """Every function node needs a column somewhere below it: a literal-only (sub)expression is not evaluated here."""
    if tree[0] in _LEAVES:
        return
    if not expr_columns(tree):
        raise ValueError("literal-only expression %s: an expression needs a column operand" % expr_name(tree))
    for a in tree[1]:
        _check_expr(a)


def parse_expression(text):
    """The canonical tree of an aggregation's argument: a column, or an arithmetic expression in function form
    (ADD / SUB / MULT / DIV, aliases PLUS / MINUS / TIMES / DIVIDE), infix (+ - * / with the usual precedence and
    parentheses), nested, with numeric literals.  ValueError for anything else."""
    p = _Parser(text)
    tree = p.arith()
    if p.peek()[0] is not None:
        raise ValueError("cannot parse expression %r near %r" % (text, p.peek()[1]))
    if tree[0] == "lit":
        raise ValueError("literal-only expression %s: an expression needs a column operand" % text)
    _number(tree, "an aggregation's argument")
    _check_expr(tree)
    check_expr_limits(tree)
    return tree


_LIKE_ESCAPED = "\\^$.{}[]()*+?|<>-&/"  # RegexpPatternConverterUtils.java:29-31, in its order: the backslash first


def like_to_regexp_like(like_pattern):
    """RegexpPatternConverterUtils.likeToRegexpLike (:36-49): each regex metacharacter is backslash-escaped, then '_'
    becomes '.' and '%' becomes '.*', and the result is wrapped in ^...$.  A LIKE wildcard cannot be escaped."""
    out = like_pattern
    for c in _LIKE_ESCAPED:
        out = out.replace(c, "\\" + c)
    return "^" + out.replace("_", ".").replace("%", ".*") + "$"


def check_regexp_pattern(pattern):
    """ValueError unless `pattern` is inside the subset of java.util.regex that REGEXP_LIKE accepts (include/pinotgpu.h,
    PGPU_PRED_REGEXP_LIKE): the library's own compiler decides, on the host, so that this layer and a plan never differ.
    Returns (states, byte classes, table bytes) of the pattern's DFA."""
    if not isinstance(pattern, str):
        raise ValueError("REGEXP_LIKE pattern %r is no string literal" % (pattern,))
    try:
        raw = pattern.encode("ascii")
    except UnicodeEncodeError:
        raise ValueError("REGEXP_LIKE pattern %r: a non-ASCII character in the pattern" % (pattern,))
    if b"\0" in raw:
        raise ValueError("REGEXP_LIKE pattern %r: a NUL character in the pattern" % (pattern,))
    try:
        return L.regex_check(raw)
    except L.UnsupportedQueryError as e:
        raise ValueError("REGEXP_LIKE pattern %r: %s" % (pattern, e))


class Predicate:
    def __init__(self, ptype, column, values, lower_inclusive=True, upper_inclusive=True):
        self.type = ptype
        self.column = column
        self.values = [str(v) for v in values]
        self.lower_inclusive = bool(lower_inclusive)
        self.upper_inclusive = bool(upper_inclusive)

    @staticmethod
    def eq(col, v):
        return Predicate(EQ, col, [v])

    @staticmethod
    def not_eq(col, v):
        return Predicate(NOT_EQ, col, [v])

    @staticmethod
    def in_(col, vals):
        return Predicate(IN, col, list(vals))

    @staticmethod
    def not_in(col, vals):
        return Predicate(NOT_IN, col, list(vals))

    @staticmethod
    def range(col, lower=UNBOUNDED, upper=UNBOUNDED, lower_inclusive=True, upper_inclusive=True):
        return Predicate(RANGE, col, [lower, upper], lower_inclusive, upper_inclusive)

    @staticmethod
    def regexp_like(col, pattern):
        """REGEXP_LIKE(col, pattern) on a STRING dictionary column; ValueError for a pattern outside the subset."""
        check_regexp_pattern(pattern)
        return Predicate(REGEXP_LIKE, col, [pattern])

    def __repr__(self):
        return "Predicate(%s %s %r)" % (self.column, self.type, self.values)


class FilterContext:
    AND, OR, NOT, PREDICATE = "AND", "OR", "NOT", "PREDICATE"

    def __init__(self, ftype, children=None, predicate=None):
        self.type = ftype
        self.children = children or []
        self.predicate = predicate

    @staticmethod
    def and_(*children):
        return FilterContext(FilterContext.AND, list(children))

    @staticmethod
    def or_(*children):
        return FilterContext(FilterContext.OR, list(children))

    @staticmethod
    def not_(child):
        return FilterContext(FilterContext.NOT, [child])

    @staticmethod
    def pred(p):
        return FilterContext(FilterContext.PREDICATE, predicate=p)

    def postfix(self, preds, ops):
        """Flattens to a postfix program (predicates numbered in left-to-right order)."""
        if self.type == FilterContext.PREDICATE:
            preds.append(self.predicate)
            ops.append((L.OP_PRED, len(preds) - 1))
        elif self.type == FilterContext.NOT:
            self.children[0].postfix(preds, ops)
            ops.append((L.OP_NOT, 0))
        else:
            for c in self.children:
                c.postfix(preds, ops)
            ops.append((L.OP_AND if self.type == FilterContext.AND else L.OP_OR, len(self.children)))


class QueryContext:
    def __init__(self, group_by, aggregations, filter=None, num_groups_limit=DEFAULT_NUM_GROUPS_LIMIT,
                 use_star_tree=True, select=None, order_by=None, limit=DEFAULT_LIMIT,
                 min_server_group_trim_size=DEFAULT_MIN_SERVER_GROUP_TRIM_SIZE,
                 group_trim_threshold=DEFAULT_GROUP_TRIM_THRESHOLD, sql_group_by=False, exact_fp_sum=False,
                 expressions=None):
        self.filter = filter
        # bit-reproducible FLOAT / DOUBLE SUM / AVG (PGPU_OPT_EXACT_FP_SUM): fixed-point digits summed as integers,
        # rounded once -- the same bits in every run, segment layout and accumulator mode (GpuPlan.fp_sum_format)
        self.exact_fp_sum = exact_fp_sum
        # queryOptions groupByMode=sql: GroupByOrderByCombineOperator (no 2 x numGroupsLimit inter-segment cap)
        self.sql_group_by = sql_group_by
        self.use_star_tree = use_star_tree  # debug option useStarTree (StarTreeUtils.java:51-59)
        self.group_by = list(group_by)
        # expressions: {function-form name: canonical tree} of the aggregation arguments that are expressions, as the
        # parser found them -- every other name is a column, whatever characters it has (a quoted identifier).  None
        # (a query built by hand): an argument, or a predicate's column, with one of ( ) + - * / is read as an
        # expression's text.
        # A group_by entry that is a key of the given `expressions` is a group-by expression (GROUP BY a + b, kept as
        # its function-form name add(a,b): parse_query(..., group_by_expressions=True)); a bare "a+b" is not parsed here.
        sniff = expressions is None
        for c in self.group_by:
            if sniff and is_expression(c):
                raise ValueError("expression %r in GROUP BY: expressions are supported inside aggregations only "
                                 "(parse_query(..., group_by_expressions=True) reads them in GROUP BY; a query built by "
                                 "hand names the expression's function form and gives its tree in `expressions`)" % (c,))
        # (fn, column) or, for the exact percentile, ("PERCENTILE", column, percentile); kept as (canonical name, column).
        # An argument that is an arithmetic expression (SUM(price * qty)) is kept as its canonical function-form name
        # (mult(price,qty)); expressions: name -> canonical tree.  Equal expressions share one name, so one virtual column.
        self.expressions = dict(expressions or {})
        self.aggregations = []
        for a in aggregations:
            col = a[1]
            if sniff and is_expression(col):
                tree = parse_expression(col)
                col = expr_name(tree)
                if tree[0] != "col":
                    self.expressions[col] = tree
            self.aggregations.append((function_name(a[0], *a[2:]), col))
        # a predicate on an expression (WHERE price * qty > 1000): its column is the canonical name too -- in a copy of
        # the filter tree, the caller's FilterContext and Predicate objects stay as they were given
        if sniff and filter is not None:
            self.filter = self._canonical_filter(filter)
        self.num_groups_limit = num_groups_limit
        # SQL-mode parts (QueryContext.getSelectExpressions / getOrderByExpressions / getLimit): the SELECT list as
        # ('col', name) / ('agg', FN, col), ORDER BY as [(expr, ascending)], LIMIT; the combine's trim options
        # (InstancePlanMakerImplV2.java:64-84)
        self.select = list(select) if select is not None else \
            [("col", c) for c in self.group_by] + [("agg", fn, col) for fn, col in self.aggregations]
        self.order_by = list(order_by or [])
        self.limit = limit
        self.min_server_group_trim_size = min_server_group_trim_size
        self.group_trim_threshold = group_trim_threshold
        # QueryContext.getEndTimeMs: absolute deadline (ms since the epoch), 0 = none (set_timeout)
        self.end_time_ms = 0
        # the executions record HIP timing events for GpuPlan.timing_us (PGPU_OPT_TIMING; off for serving)
        self.timing = False

    def _canonical_filter(self, f):
        """f with every predicate column that reads as an expression replaced by its canonical name (the trees go into
        self.expressions): new nodes where something changes below them, the given ones elsewhere."""
        if f.type == FilterContext.PREDICATE:
            p = f.predicate
            if not is_expression(p.column):
                return f
            tree = parse_expression(p.column)
            name = expr_name(tree)
            if tree[0] != "col":
                self.expressions[name] = tree
            q = Predicate(p.type, name, p.values, p.lower_inclusive, p.upper_inclusive)
            return FilterContext.pred(q)
        kids = [self._canonical_filter(k) for k in f.children]
        if all(k is c for k, c in zip(kids, f.children)):
            return f
        return FilterContext(f.type, kids)

    def set_timeout(self, timeout_ms):
        """End time = now + timeout_ms (the broker's arrival time + queryOptions timeoutMs,
        QueryContext.setEndTimeMs); None clears it.  Past it the GPU path raises QueryTimeoutError."""
        self.end_time_ms = 0 if timeout_ms is None else int(time.time() * 1000) + int(timeout_ms)
        return self

    def group_expr(self, column):
        """The tree of group-by entry `column` if it is an expression, else None."""
        return self.expressions.get(column) if column in self.group_by else None

    def expr_ref(self, expr):
        """(kind, index) of a SELECT / ORDER BY expression over the result: (0, group-by position) or
        (1, aggregation position)."""
        if expr[0] == "col":
            return L.ORDER_GROUP_BY, self.group_by.index(expr[1])
        return L.ORDER_AGGREGATION, self.aggregations.index((function_name(expr[1]), expr[2]))

    def sql_trim_c(self):
        """The SQL-mode combine / reduce options as pgpu_sql_trim (keepalive, struct)."""
        ob = (L.OrderByC * max(len(self.order_by), 1))()
        for i, (e, asc) in enumerate(self.order_by):
            ob[i].kind, ob[i].index = self.expr_ref(e)
            ob[i].ascending = int(asc)
        sel = (L.OrderByC * max(len(self.select), 1))()
        for i, e in enumerate(self.select):
            sel[i].kind, sel[i].index = self.expr_ref(e)
        t = L.SqlTrimC(len(self.order_by), ob, self.limit, self.min_server_group_trim_size, self.group_trim_threshold,
                       len(self.select), sel)
        return (ob, sel), t

    def columns(self):
        cols = []
        if self.filter is not None:
            preds = []
            self.filter.postfix(preds, [])
            for p in preds:
                cols += expr_columns(self.expressions[p.column]) if p.column in self.expressions else [p.column]
        for c in self.group_by:  # (a group-by expression reads its operands)
            cols += expr_columns(self.expressions[c]) if c in self.expressions else [c]
        for _, c in self.aggregations:
            cols += expr_columns(self.expressions[c]) if c in self.expressions else [c] * (c != "*")
        out = []
        for c in cols:
            if c not in out:
                out.append(c)
        return out

    # ---- JSON form used by tests/golden/kat_sv.json
    @staticmethod
    def filter_from_json(j):
        if j is None:
            return None
        if "and" in j:
            return FilterContext.and_(*[QueryContext.filter_from_json(c) for c in j["and"]])
        if "or" in j:
            return FilterContext.or_(*[QueryContext.filter_from_json(c) for c in j["or"]])
        if "not" in j:
            return FilterContext.not_(QueryContext.filter_from_json(j["not"]))
        t = j["pred"]
        if t in (EQ, NOT_EQ):
            return FilterContext.pred(Predicate(t, j["col"], [j["value"]]))
        if t in (IN, NOT_IN):
            return FilterContext.pred(Predicate(t, j["col"], j["values"]))
        return FilterContext.pred(Predicate.range(j["col"], j["lower"], j["upper"], j.get("li", True), j.get("ui", True)))

    # ---- C ABI form
    def to_c(self, column_index):
        """Returns (QueryC, keepalive) for a table whose column name -> index map is `column_index`.  The ctypes
        form is built once per (query, table) and reused; options are refreshed on every call."""
        cache = self.__dict__.get("_c_cache")
        if cache is not None and cache[0] is column_index and cache[1] == self.num_groups_limit:
            q, keep = cache[2], cache[3]
            q.options = self._options()
            q.end_time_ms = getattr(self, "end_time_ms", 0)
            return q, keep
        q, keep = self._build_c(column_index)
        self._c_cache = (column_index, self.num_groups_limit, q, keep)
        return q, keep

    def _options(self):
        return (0 if getattr(self, "use_star_tree", True) else L.OPT_NO_STAR_TREE) | \
            (L.OPT_SQL_GROUP_BY if getattr(self, "sql_group_by", False) else 0) | \
            (L.OPT_NO_PLAN_CACHE if getattr(self, "no_plan_cache", False) else 0) | \
            (L.OPT_TIMING if getattr(self, "timing", False) else 0) | \
            (L.OPT_EXACT_FP_SUM if getattr(self, "exact_fp_sum", False) else 0)

    def _build_c(self, column_index):
        keep = []
        preds, ops = [], []
        if self.filter is not None:
            self.filter.postfix(preds, ops)
        pc = (L.PredicateC * max(len(preds), 1))()
        for i, p in enumerate(preds):
            if p.column not in column_index:
                raise KeyError("unknown column %r" % p.column)
            vals = (ctypes.c_char_p * max(len(p.values), 1))(*[v.encode() for v in p.values])
            keep.append(vals)
            pc[i].type = _PRED_CODE[p.type]
            pc[i].column = column_index[p.column]
            pc[i].num_values = len(p.values)
            pc[i].values = ctypes.cast(vals, L.c_char_pp)
            pc[i].lower_inclusive = int(p.lower_inclusive)
            pc[i].upper_inclusive = int(p.upper_inclusive)
        oc = (L.FilterOpC * max(len(ops), 1))()
        for i, (o, a) in enumerate(ops):
            oc[i].op, oc[i].arg = o, a
        # (a group-by expression: GpuTable registers it under ("group", name) -- the aggregation's virtual column of the
        # same name, SUM(a*b) .. GROUP BY a*b, is another index)
        gb = (ctypes.c_int32 * max(len(self.group_by), 1))(
            *[column_index[("group", c) if c in self.expressions else c] for c in self.group_by])
        ac = (L.AggC * max(len(self.aggregations), 1))()
        for i, (fn, col) in enumerate(self.aggregations):
            p_e4 = percentile_e4(fn)
            if p_e4 is not None:  # pgpu_agg.fn: the code in bits 0..7, the percentile above (PGPU_AGG_PERCENTILE_OF)
                ac[i].fn = L.AGG_PERCENTILE | (p_e4 << 8)
            elif fn not in AGG_FUNCTIONS:
                raise L.UnsupportedQueryError(L.PGPU_ERR_UNSUPPORTED, "aggregation %s" % fn)
            else:
                ac[i].fn = AGG_FUNCTIONS[fn]
            if col in self.expressions and ac[i].fn == L.AGG_COUNT:
                ac[i].column = -1  # COUNT(expr) is COUNT
            elif col == "*":
                ac[i].column = -1
            elif col not in column_index:  # (an expression: GpuTable registers it, then the name is a column)
                raise KeyError("unknown column %r" % col)
            else:
                ac[i].column = column_index[col]
        q = L.QueryC()
        q.num_predicates = len(preds)
        q.num_filter_ops = len(ops)
        q.predicates = pc
        q.filter = oc
        q.num_group_by = len(self.group_by)
        q.group_by = gb
        q.num_aggs = len(self.aggregations)
        q.aggs = ac
        q.num_groups_limit = self.num_groups_limit
        q.options = self._options()
        q.end_time_ms = getattr(self, "end_time_ms", 0)
        keep += [pc, oc, gb, ac]
        return q, keep


# ================================================================================ SQL / PQL subset parser
# (a number's sign is a token of its own, so that a-1 is a subtraction: _Parser.literal / arith put it back)
_TOKEN = re.compile(r"\s*(?:(?P<num>\d+(?:\.\d+)?(?:[eE][+-]?\d+)?)|(?P<str>'(?:[^']|'')*')|"
                    r"(?P<id>[A-Za-z_][A-Za-z0-9_.$]*|\"[^\"]+\")|(?P<op><=|>=|<>|!=|=|<|>|\(|\)|,|\*|\+|-|/))")


def _tokenize(s):
    pos, out = 0, []
    s = s.strip().rstrip(";")
    while pos < len(s):
        m = _TOKEN.match(s, pos)
        if not m or m.end() == pos:
            if s[pos:].strip() == "":
                break
            raise ValueError("cannot parse near %r" % s[pos:pos + 20])
        pos = m.end()
        if m.group("num") is not None:
            out.append(("lit", m.group("num")))
        elif m.group("str") is not None:
            out.append(("lit", m.group("str")[1:-1].replace("''", "'")))
        elif m.group("id") is not None:
            out.append(("id", m.group("id").strip('"')))
        else:
            out.append(("op", m.group("op")))
    return out


_ARITH_OPS = (("op", "+"), ("op", "-"), ("op", "*"), ("op", "/"))


class _Parser:
    def __init__(self, sql, filter_expressions=False, group_by_expressions=False):
        self.t = _tokenize(sql)
        self.i = 0
        # GROUP BY a + b (parse_query): function-form name -> tree of the expressions met in GROUP BY and, in SELECT and
        # ORDER BY, of the items that are expressions over columns (named_exprs: their names, matched to the GROUP BY
        # entries once those are known)
        self.group_by_expressions = group_by_expressions
        self.group_exprs = {}
        self.named_exprs = []
        # function-form name -> tree of the aggregation arguments and predicate left-hand sides that are expressions
        self.exprs = {}
        self.filter_expressions = filter_expressions  # WHERE price * qty > 1000 (parse_query)

    def peek(self, k=0):
        return self.t[self.i + k] if self.i + k < len(self.t) else (None, None)

    def kw(self, *words):
        tok = self.peek()
        return tok[0] == "id" and tok[1].upper() in words

    def take(self, kind=None, value=None):
        tok = self.peek()
        if tok[0] is None or (kind and tok[0] != kind) or (value and str(tok[1]).upper() != value):
            raise ValueError("expected %s %s, got %r" % (kind, value, tok))
        self.i += 1
        return tok[1]

    def group_expr_ahead(self):
        """Whether the SELECT / ORDER BY item at hand is an expression over columns, not an aggregation or a plain
        column: a CASE, a parenthesis, a number, a transform function (whose names no aggregation function has), or a
        column followed by an arithmetic operator."""
        tok = self.peek()
        if self.case_ahead() or tok in (("op", "("), ("op", "-")) or tok[0] == "lit":
            return True
        if tok[0] != "id":
            return False
        if self.peek(1) == ("op", "("):
            up = tok[1].upper()
            key = transform_function_name(up)
            return up in _EXPR_FUNCTIONS or up in _CMP_FUNCTIONS or up in ("AND", "OR", "CASE") or key == "MOD" or \
                key in _MATH_FUNCTIONS or key in _TIME_FUNCTIONS or key in _DECLINED_FUNCTIONS
        return self.peek(1) in _ARITH_OPS

    def group_expr_item(self):
        """A GROUP BY item, or a SELECT / ORDER BY item that group_expr_ahead: the grammar and limits of an
        aggregation's argument, kept as its canonical function-form name."""
        tree = self.arith_checked()
        name = expr_name(tree)
        if tree[0] != "col":
            self.group_exprs[name] = tree
        return name

    def select_list_item(self):
        tok = self.peek()
        if self.group_by_expressions and self.group_expr_ahead():
            name = self.group_expr_item()
            if name in self.group_exprs:
                self.named_exprs.append(name)
            return ("col", name)
        if tok[0] == "id" and self.peek(1) == ("op", "("):
            fn = self.take("id")
            self.take("op", "(")
            col = "*" if self.peek() == ("op", "*") else None
            if col:
                self.take("op", "*")
            else:  # a column, or an arithmetic expression kept as its canonical function-form name
                tree = self.arith_checked()
                col = expr_name(tree)
                if tree[0] != "col":
                    self.exprs[col] = tree
            arg = None
            if self.peek() == ("op", ","):  # PERCENTILE(x, 95) / PERCENTILE(x, '95')
                self.take("op", ",")
                arg = self.literal()
            self.take("op", ")")
            return ("agg", function_name(fn, arg), col)
        return ("col", self.take("id"))

    def select_list(self):
        items = []
        while True:
            items.append(self.select_list_item())
            if self.peek() == ("op", ","):
                self.take("op", ",")
                continue
            return items

    def literal(self):
        tok = self.peek()
        if tok == ("op", "-") and self.peek(1)[0] == "lit":  # a negative number
            self.i += 2
            return "-" + self.peek(-1)[1]
        if tok[0] not in ("lit", "id"):
            raise ValueError("literal expected, got %r" % (tok,))
        self.i += 1
        return tok[1]

    # ---- an aggregation's argument: arith := term (+|- term)*, term := factor (*|/ factor)*,
    # factor := [-] number | FN ( arith , ... ) | column | ( arith )
    def arith_checked(self):
        tree = self.arith()
        if tree[0] == "lit":
            raise ValueError("literal-only expression %s: an expression needs a column operand" % tree[1])
        _number(tree, "an aggregation's argument or a predicate's left-hand side")
        _check_expr(tree)
        check_expr_limits(tree)
        return tree

    def arith(self):
        left = self.term()
        while self.peek() in (("op", "+"), ("op", "-")):
            op = self.take("op")
            left = expr_node("ADD" if op == "+" else "SUB", [left, self.term()])
        return left

    def term(self):
        left = self.factor()
        while self.peek() in (("op", "*"), ("op", "/")):
            op = self.take("op")
            left = expr_node("MULT" if op == "*" else "DIV", [left, self.factor()])
        return left

    def factor(self):
        tok = self.peek()
        if tok == ("op", "("):
            self.take("op", "(")
            e = self.arith()
            self.take("op", ")")
            return e
        if tok == ("op", "-"):  # unary minus on a literal
            self.take("op", "-")
            if self.peek()[0] != "lit":
                raise ValueError("unary minus is supported on a numeric literal only, got %r" % (self.peek(),))
            return expr_literal("-" + self.take("lit"))
        if tok[0] == "lit":
            return expr_literal(self.take("lit"))
        if self.case_ahead():
            return self.case()
        if tok[0] == "id" and self.peek(1) == ("op", "("):
            fn = self.take("id")
            self.take("op", "(")
            # (the unit and format arguments of the time functions are string literals, which arithmetic has none of)
            strings = transform_function_name(fn) in _TIME_FUNCTIONS
            args = [self.arith()]
            while self.peek() == ("op", ","):
                self.take("op", ",")
                args.append(("str", self.take("lit")) if strings and self.peek()[0] == "lit" else self.arith())
            self.take("op", ")")
            return expr_node(fn, args)
        return ("col", self.take("id"))

    # ---- CASE WHEN cond THEN arith (WHEN cond THEN arith)* ELSE arith END; cond := conj (OR conj)*,
    # conj := ctest (AND ctest)*, ctest := ( cond ) | arith cmp arith, cmp one of = != <> < <= > >=
    def case_ahead(self):
        return self.kw("CASE") and self.peek(1)[0] == "id" and self.peek(1)[1].upper() == "WHEN"

    def case(self):
        self.take("id", "CASE")
        whens, thens, els = [], [], None
        while self.kw("WHEN"):
            self.take("id")
            whens.append(self.cond())
            self.take("id", "THEN")
            thens.append(self.arith())
        if not whens:
            raise ValueError("CASE: WHEN expected, got %r (the simple form CASE x WHEN v is not supported)" % (self.peek(),))
        if self.kw("ELSE"):
            self.take("id")
            els = self.arith()
        self.take("id", "END")
        return case_node(whens, thens, els)

    def cond(self):
        kids = [self.cond_and()]
        while self.kw("OR"):
            self.take("id")
            kids.append(self.cond_and())
        return kids[0] if len(kids) == 1 else logic_node("or", kids)

    def cond_and(self):
        kids = [self.cond_test()]
        while self.kw("AND"):
            self.take("id")
            kids.append(self.cond_test())
        return kids[0] if len(kids) == 1 else logic_node("and", kids)

    def cond_test(self):
        if self.peek() == ("op", "("):  # a condition in parentheses, or -- (a + b) * 2 > 3 -- an arithmetic operand
            mark = self.i
            try:
                self.take("op", "(")
                c = self.cond()
                self.take("op", ")")
                if self.peek() not in _ARITH_OPS and not (self.peek()[0] == "op" and self.peek()[1] in _CMP_SQL):
                    return c
            except ValueError:
                pass
            self.i = mark
        left = self.arith()
        if _is_bool(left):  # the function form: greater_than(a, 1), and(.., ..)
            return left
        if self.kw("IN", "NOT", "BETWEEN"):
            raise ValueError("%s inside a CASE WHEN is not supported: a condition is a comparison (= != <> < <= > >=), "
                             "AND, OR" % self.peek()[1].upper())
        tok = self.peek()
        if tok[0] != "op" or tok[1] not in _CMP_SQL:
            raise ValueError("comparison expected in a CASE WHEN, got %r" % (tok,))
        self.take("op")
        return cmp_node(_CMP_SQL[tok[1]], left, self.arith())

    def rhs_literal(self, lhs):
        """A predicate's right-hand side: a literal.  After an expression a name there is a column (a * b < c), which
        the reference rewrites in its broker and this layer does not model.  After a plain column a name stays the
        literal it has always been ("x" in double quotes, true): filter_expressions changes nothing for plain predicates."""
        if lhs in self.exprs and self.peek()[0] == "id":
            raise ValueError("column %r on the right-hand side of %s: an expression is compared with a literal"
                             % (self.peek()[1], lhs))
        return self.literal()

    def predicate_lhs(self):
        """A predicate's left-hand side: a column, or -- with filter_expressions -- an arithmetic expression, kept as
        its canonical function-form name with the tree in self.exprs (the reference's ExpressionFilterOperator)."""
        if not self.filter_expressions:
            col = self.take("id")
            if self.peek() in (("op", "("),) + _ARITH_OPS:
                raise ValueError("expression in WHERE near %r: expressions are supported inside aggregations only "
                                 "(parse_query(..., filter_expressions=True) reads them in WHERE too)" % col)
            return col
        tok = self.peek()
        if tok[0] == "id" and self.peek(1) not in (("op", "("),) + _ARITH_OPS and not self.case_ahead():
            return self.take("id")  # a plain column
        tree = self.arith_checked()
        name = expr_name(tree)
        if tree[0] != "col":
            self.exprs[name] = tree
        return name

    def expr_or(self):
        kids = [self.expr_and()]
        while self.kw("OR"):
            self.take("id")
            kids.append(self.expr_and())
        return kids[0] if len(kids) == 1 else FilterContext.or_(*kids)

    def expr_and(self):
        kids = [self.expr_not()]
        while self.kw("AND"):
            self.take("id")
            kids.append(self.expr_not())
        return kids[0] if len(kids) == 1 else FilterContext.and_(*kids)

    def expr_not(self):
        if self.kw("NOT"):
            self.take("id")
            return FilterContext.not_(self.expr_not())
        if self.peek() == ("op", "("):
            # a boolean group first; where that fails -- (a + b) * 2 > 3 -- the term is re-read from the same token as
            # the arithmetic left-hand side of a comparison
            mark, exprs = self.i, dict(self.exprs)
            try:
                self.take("op", "(")
                e = self.expr_or()
                self.take("op", ")")
                if self.peek() in _ARITH_OPS and self.filter_expressions:
                    raise ValueError("a boolean group is no operand of %r" % (self.peek()[1],))
                return e
            except ValueError as first:
                if not self.filter_expressions:
                    raise
                # the error of whichever reading got further is the one about what the user wrote: a group that
                # lacks its ")" fails at the end, its re-read as arithmetic at the first comparison inside it
                reached = self.i
                self.i, self.exprs = mark, exprs
                try:
                    return self.predicate()
                except ValueError:
                    if self.i > reached:
                        raise
                    raise first
        return self.predicate()

    def predicate(self):
        f = self.predicate_of()
        if f.type != FilterContext.PREDICATE:  # col NOT LIKE 'p': NOT over the predicate
            return f
        tree = self.exprs.get(f.predicate.column)
        # a time function on the left is LONG whatever its column is (a CASE's type waits for the column types: query_c)
        if tree is not None and tree[0] in ("timeconvert", "datetimeconvert"):
            f.predicate = long_predicate(f.predicate)
        return f

    def pattern_literal(self, what):
        if self.peek()[0] != "lit":
            raise ValueError("%s: the pattern must be a literal, got %r" % (what, self.peek()[1]))
        return self.take("lit")

    def regexp_column(self, col, what):
        if col in self.exprs:
            raise ValueError("%s over the expression %s: the left-hand side must be a column" % (what, col))
        return col

    def predicate_of(self):
        if self.kw("REGEXP_LIKE") and self.peek(1) == ("op", "("):
            self.take("id")
            self.take("op", "(")
            if self.peek()[0] != "id" or self.peek(1) != ("op", ","):
                raise ValueError("REGEXP_LIKE: the first argument must be a column, not an expression or a literal")
            col = self.take("id")
            self.take("op", ",")
            pattern = self.pattern_literal("REGEXP_LIKE(%s, ..)" % col)
            self.take("op", ")")
            return FilterContext.pred(Predicate.regexp_like(col, pattern))
        col = self.predicate_lhs()
        if self.kw("LIKE") or (self.kw("NOT") and self.peek(1)[0] == "id" and self.peek(1)[1].upper() == "LIKE"):
            negate = self.kw("NOT")
            if negate:
                self.take("id")
            self.take("id")
            self.regexp_column(col, "LIKE")
            pattern = like_to_regexp_like(self.pattern_literal("%s LIKE" % col))
            f = FilterContext.pred(Predicate.regexp_like(col, pattern))
            return FilterContext.not_(f) if negate else f
        if self.kw("BETWEEN"):
            self.take("id")
            lo = self.rhs_literal(col)
            self.take("id", "AND")
            hi = self.rhs_literal(col)
            return FilterContext.pred(Predicate.range(col, lo, hi, True, True))
        negate = False
        if self.kw("NOT"):
            self.take("id")
            negate = True
        if self.kw("IN"):
            self.take("id")
            self.take("op", "(")
            vals = [self.rhs_literal(col)]
            while self.peek() == ("op", ","):
                self.take("op", ",")
                vals.append(self.rhs_literal(col))
            self.take("op", ")")
            return FilterContext.pred(Predicate.not_in(col, vals) if negate else Predicate.in_(col, vals))
        op = self.take("op")
        v = self.rhs_literal(col)
        if op == "=":
            return FilterContext.pred(Predicate.eq(col, v))
        if op in ("!=", "<>"):
            return FilterContext.pred(Predicate.not_eq(col, v))
        if op == ">":
            return FilterContext.pred(Predicate.range(col, v, UNBOUNDED, False, False))
        if op == ">=":
            return FilterContext.pred(Predicate.range(col, v, UNBOUNDED, True, False))
        if op == "<":
            return FilterContext.pred(Predicate.range(col, UNBOUNDED, v, False, False))
        if op == "<=":
            return FilterContext.pred(Predicate.range(col, UNBOUNDED, v, False, True))
        raise ValueError("unsupported operator %s" % op)


def parse_query(sql, num_groups_limit=DEFAULT_NUM_GROUPS_LIMIT, exact_fp_sum=False, filter_expressions=False,
                group_by_expressions=False):
    """Parses `SELECT cols / aggs FROM t [WHERE ...] [GROUP BY cols] [ORDER BY expr [ASC|DESC], ...]
    [TOP n | LIMIT n]`.  Aggregations that appear only in ORDER BY are computed as well (Pinot's hidden
    aggregations) but not selected.  exact_fp_sum: the query option of the same name (QueryContext).
    filter_expressions: a predicate's left-hand side may be an arithmetic expression (WHERE price * qty > 1000,
    WHERE ADD(a, b) BETWEEN 1 AND 5, IN / NOT IN; the grammar and limits of an aggregation's argument); the right-hand
    side stays a literal.  GpuTable parses its SQL strings with it on.  The default is off only because
    tests/test_expr_agg_cpu.py pins ValueError for such strings under the default call.
    group_by_expressions: a GROUP BY item may be an expression -- GROUP BY a + b, GROUP BY CASE WHEN age < 18 THEN 0 ELSE
    1 END, GROUP BY add(a, b): the grammar, limits and typing of an aggregation's argument.  It is kept as its canonical
    function-form name (add(a,b)) with the tree in QueryContext.expressions; a SELECT or ORDER BY item that is such an
    expression, in any accepted spelling, is matched to the GROUP BY entry by that name and becomes ("col", name), and
    one that matches none is a ValueError.  GpuTable parses its SQL strings with it on; the default is off for the
    same reason as filter_expressions."""
    p = _Parser(sql, filter_expressions, group_by_expressions)
    p.take("id", "SELECT")
    items = p.select_list()
    p.take("id", "FROM")
    p.take("id")
    flt = None
    if p.kw("WHERE"):
        p.take("id")
        flt = p.expr_or()
    group_by = []
    if p.kw("GROUP"):
        p.take("id")
        p.take("id", "BY")
        def group_by_column():
            if group_by_expressions:
                return p.group_expr_item()
            if p.case_ahead():
                raise ValueError("expression in GROUP BY near 'CASE': expressions are supported inside aggregations only")
            col = p.take("id")
            if p.peek() in (("op", "("), ("op", "+"), ("op", "-"), ("op", "*"), ("op", "/")):
                raise ValueError("expression in GROUP BY near %r: expressions are supported inside aggregations only" % col)
            return col
        group_by.append(group_by_column())
        while p.peek() == ("op", ","):
            p.take("op", ",")
            group_by.append(group_by_column())
    order_by, limit = [], DEFAULT_LIMIT
    if p.kw("ORDER"):
        p.take("id")
        p.take("id", "BY")
        while True:
            e = p.select_list_item()
            asc = True
            if p.kw("ASC", "DESC"):
                asc = p.take("id").upper() == "ASC"
            order_by.append((e if e[0] == "col" else ("agg", e[1], e[2]), asc))
            if p.peek() != ("op", ","):
                break
            p.take("op", ",")
    if p.kw("TOP", "LIMIT"):
        p.take("id")
        limit = int(p.literal())
    for name in p.named_exprs:
        if name not in group_by:
            raise ValueError("expression %s in SELECT / ORDER BY is no GROUP BY expression of the query" % name)
    exprs = dict(p.exprs)
    exprs.update({c: p.group_exprs[c] for c in group_by if c in p.group_exprs})
    select = [("col", it[1]) if it[0] == "col" else ("agg", it[1], it[2]) for it in items]
    aggs = []
    for e in [x for x in select if x[0] == "agg"] + [e for e, _ in order_by if e[0] == "agg"]:
        if (e[1], e[2]) not in aggs:
            aggs.append((e[1], e[2]))
    return QueryContext(group_by, aggs, flt, num_groups_limit, select=select, order_by=order_by, limit=limit,
                        exact_fp_sum=exact_fp_sum, expressions=exprs)
