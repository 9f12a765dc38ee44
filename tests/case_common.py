"""The yardstick of the conditional-expression tests (CASE WHEN inside aggregations and WHERE): the reference's typing
rules restated directly over typed numpy arrays -- np.float32 rounding of FLOAT literals, int64 compares of integer
pairs, Double.compare's total order by key for everything else, the CASE result type folded over ELSE and the THENs.  It
walks the canonical tree and never calls pinot_amd.query.expr_program (or its helpers literal_type / expr_type), so a
mistake in the compiler cannot agree with itself.

Columns are numpy arrays whose dtype is the column's type: int32 INT, int64 LONG, float32 FLOAT, float64 DOUBLE."""
import re

import numpy as np

import expr_common as E

INT, LONG, FLOAT, DOUBLE = "INT", "LONG", "FLOAT", "DOUBLE"
DTYPE = {INT: np.int32, LONG: np.int64, FLOAT: np.float32, DOUBLE: np.float64}
CMP = ("equals", "not_equals", "greater_than", "greater_than_or_equal", "less_than", "less_than_or_equal")
I64_MAX = np.int64(2 ** 63 - 1)


def typed(cols, schema):
    """cols with every numeric column as an array of its schema type's dtype."""
    types = dict(schema)
    return {c: np.asarray(v).astype(DTYPE[types[c]]) for c, v in cols.items() if types[c] in DTYPE}


def col_type(a):
    return {np.dtype(np.int32): INT, np.dtype(np.int64): LONG, np.dtype(np.float32): FLOAT,
            np.dtype(np.float64): DOUBLE}[a.dtype]


def lit_type(text):
    """NumberUtils.createNumber of the literal's text on the server."""
    if re.fullmatch(r"-?\d+", text):
        v = int(text)
        assert -2 ** 63 <= v < 2 ** 63
        return INT if -2 ** 31 <= v < 2 ** 31 else LONG
    decimals = len(re.fullmatch(r"-?\d+\.(\d+)(E-?\d+)?", text).group(1))
    with np.errstate(over="ignore"):
        f = np.float32(float(text))
    if decimals <= 7 and np.isfinite(f) and not (f == 0 and float(text) != 0):
        return FLOAT
    assert decimals <= 16
    return DOUBLE


def fold(a, b):
    return a if a == b else LONG if {a, b} == {INT, LONG} else DOUBLE


def node_type(t, cols):
    if t[0] == "col":
        return col_type(cols[t[1]])
    if t[0] == "lit":
        return lit_type(t[1])
    if t[0] == "case":
        n = (len(t[1]) - 1) // 2
        r = node_type(t[1][2 * n], cols)
        for x in t[1][n:2 * n]:
            r = fold(r, node_type(x, cols))
        return r
    assert t[0] in ("add", "sub", "mult", "div"), t[0]
    return DOUBLE


def keys(v):
    """Double.compare's order as int64 keys: the bits of a positive value, a negative one's magnitude flipped, every
    NaN the canonical one."""
    v = np.asarray(v, dtype=np.float64)
    b = v.view(np.int64).copy() if v.ndim else np.array(v).reshape(1).view(np.int64).copy()
    b[np.isnan(v.reshape(b.shape))] = np.int64(E.NAN_KEY)
    return np.where(b >= 0, b, b ^ I64_MAX)


def _n(cols):
    return len(next(iter(cols.values())))


def ints(t, cols):
    """An INT / LONG typed tree's per-doc integers (int64)."""
    if t[0] == "col":
        return cols[t[1]].astype(np.int64)
    if t[0] == "lit":
        return np.full(_n(cols), int(t[1]), dtype=np.int64)
    assert t[0] == "case"
    return _select(t, cols, lambda x: ints(x, cols))


def _select(t, cols, value):
    n = (len(t[1]) - 1) // 2
    out = value(t[1][2 * n])
    for w, x in reversed(list(zip(t[1][:n], t[1][n:2 * n]))):  # the first matching WHEN wins
        out = np.where(cond(w, cols), value(x), out)
    return out


def cmp_operand(t, cols):
    """A comparison operand's doubles, a literal read as its own type."""
    if t[0] == "lit":
        ty = lit_type(t[1])
        v = float(int(t[1])) if ty in (INT, LONG) else float(np.float32(float(t[1]))) if ty == FLOAT else float(t[1])
        return np.full(_n(cols), v, dtype=np.float64)
    return doubles(t, cols)


def cond(t, cols):
    """A condition's per-doc booleans."""
    if t[0] in ("and", "or"):
        kids = [cond(k, cols) for k in t[1]]
        return np.logical_and.reduce(kids) if t[0] == "and" else np.logical_or.reduce(kids)
    a, b = t[1]
    ta, tb = node_type(a, cols), node_type(b, cols)
    assert not (ta == LONG and tb in (FLOAT, DOUBLE)) and not (tb == LONG and ta in (FLOAT, DOUBLE)), "a declined pair"
    if ta in (INT, LONG) and tb in (INT, LONG):  # Integer.compare / Long.compare
        x, y = ints(a, cols), ints(b, cols)
    else:  # Double.compare of the widened values
        x, y = keys(cmp_operand(a, cols)), keys(cmp_operand(b, cols))
    return {"equals": x == y, "not_equals": x != y, "greater_than": x > y, "greater_than_or_equal": x >= y,
            "less_than": x < y, "less_than_or_equal": x <= y}[t[0]]


def doubles(t, cols):
    """A numeric tree's per-doc doubles: what SUM / MIN / MAX read (transformToDoubleValuesSV)."""
    if t[0] == "col":
        return cols[t[1]].astype(np.float64)
    if t[0] == "lit":  # a literal inside arithmetic: Double.parseDouble
        return np.full(_n(cols), float(t[1]), dtype=np.float64)
    if t[0] == "case":
        r = node_type(t, cols)

        def branch(x):
            if x[0] != "lit":
                return doubles(x, cols)
            v = float(int(x[1])) if r in (INT, LONG) else float(np.float32(float(x[1]))) if r == FLOAT else float(x[1])
            return np.full(_n(cols), v, dtype=np.float64)
        return _select(t, cols, branch)
    assert t[0] in ("add", "sub", "mult", "div"), t[0]
    return _arith(t, lambda a: doubles(a, cols))


def eval_docs(tree, cols):
    """The per-doc doubles of a numeric tree over typed columns."""
    return np.asarray(doubles(tree, cols), dtype=np.float64)


def unrounded_docs(tree, cols):
    """eval_docs with every decimal literal as its plain double and every compare in doubles: what a compiler that
    ignored the FLOAT typing of literals would compute (the tests show their data tells the two apart)."""
    def d(t):
        if t[0] == "col":
            return cols[t[1]].astype(np.float64)
        if t[0] == "lit":
            return np.full(_n(cols), float(t[1]), dtype=np.float64)
        if t[0] == "case":
            n = (len(t[1]) - 1) // 2
            out = d(t[1][2 * n])
            for w, x in reversed(list(zip(t[1][:n], t[1][n:2 * n]))):
                out = np.where(c(w), d(x), out)
            return out
        return _arith(t, d)

    def c(t):
        if t[0] in ("and", "or"):
            kids = [c(k) for k in t[1]]
            return np.logical_and.reduce(kids) if t[0] == "and" else np.logical_or.reduce(kids)
        x, y = keys(d(t[1][0])), keys(d(t[1][1]))
        return {"equals": x == y, "not_equals": x != y, "greater_than": x > y, "greater_than_or_equal": x >= y,
                "less_than": x < y, "less_than_or_equal": x <= y}[t[0]]
    return np.asarray(d(tree), dtype=np.float64)


def _arith(t, d):
    """An arithmetic node over its arguments' doubles d(arg): one float64 operation per step, in the reference's order."""
    fn, args = t
    with np.errstate(all="ignore"):
        if fn == "sub":
            return d(args[0]) - d(args[1])
        if fn == "div":
            return d(args[0]) / d(args[1])
        acc = np.float64(0.0 if fn == "add" else 1.0)
        for a in args:
            if a[0] == "lit":
                acc = acc + np.float64(a[1]) if fn == "add" else acc * np.float64(a[1])
        for a in args:
            if a[0] != "lit":
                acc = acc + d(a) if fn == "add" else acc * d(a)
        return acc


def branch_counts(tree, cols):
    """Per CASE of the tree (outermost first): how many docs each WHEN and the ELSE select."""
    out = []

    def walk(t):
        if t[0] in ("col", "lit"):
            return
        if t[0] == "case":
            n = (len(t[1]) - 1) // 2
            left = np.ones(_n(cols), dtype=bool)
            counts = []
            for w in t[1][:n]:
                m = cond(w, cols) & left
                counts.append(int(m.sum()))
                left &= ~m
            out.append(counts + [int(left.sum())])
        for a in t[1]:
            walk(a)
    walk(tree)
    return out
