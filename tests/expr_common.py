"""Shared by the tests of expressions inside aggregations (SUM(price * qty)): the reference's recorded answers
(tests/golden/kat_transform_avg.json) and the yardstick the oracle does not have -- the canonical tree evaluated with
Python floats in the reference's order (Python floats are IEEE doubles, and Python never fuses a multiply-add), then a
sum / min / max per group in the same doubles."""
import fractions
import json
import math
import os
import struct

import numpy as np

from pinot_amd.query import parse_expression

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_TRANSFORM = json.load(open(os.path.join(HERE, "golden", "kat_transform_avg.json")))
NAN_KEY = 0x7ff8000000000000  # Double.doubleToLongBits's NaN


def bits(x):
    """The bit pattern of a double, as an unsigned integer."""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def canon_bits(x):
    """bits(), every NaN as Double.doubleToLongBits's one: which NaN an operation returns (sign, payload) is the
    machine's choice -- x86 answers 0 / 0 with the negative quiet NaN, the GPU with the positive one -- and Java
    itself only ever compares the canonical one."""
    return NAN_KEY if x != x else bits(x)


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def key(x):
    """The project's order-preserving int64 key of a double (NaN canonical): MIN / MAX compare through it."""
    b = NAN_KEY if x != x else bits(x)
    b = b - (1 << 64) if b >= 1 << 63 else b
    return b if b >= 0 else b ^ ((1 << 63) - 1)


def _div(a, b):
    """IEEE division (Python raises on a zero divisor; Java gives +-inf or NaN)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def eval_tree(tree, row):
    """One doc's value: `row` maps a column to its double.  ADD: the sum of the literal arguments from 0.0 in argument
    order, then the other arguments added in argument order (AdditionTransformFunction.java:44-82); MULT likewise from
    1.0; SUB and DIV: a op b."""
    if tree[0] == "col":
        return float(row[tree[1]])
    if tree[0] == "lit":
        return float(tree[1])
    fn, args = tree
    if fn == "sub":
        return eval_tree(args[0], row) - eval_tree(args[1], row)
    if fn == "div":
        return _div(eval_tree(args[0], row), eval_tree(args[1], row))
    acc = 0.0 if fn == "add" else 1.0
    for a in args:
        if a[0] == "lit":
            acc = acc + float(a[1]) if fn == "add" else acc * float(a[1])
    for a in args:
        if a[0] != "lit":
            v = eval_tree(a, row)
            acc = acc + v if fn == "add" else acc * v
    return acc


def column_doubles(values):
    """getDoubleValuesSV of a column: (double)value, through float32 for a FLOAT column (dtype float32)."""
    return np.asarray(values).astype(np.float64)


def eval_docs(expr, cols):
    """The per-doc doubles of expression `expr` (text or tree) over `cols` (name -> array), as a float64 array."""
    tree = parse_expression(expr) if isinstance(expr, str) else expr
    d = {c: column_doubles(v).tolist() for c, v in cols.items() if not isinstance(v, list)}
    n = len(next(iter(d.values())))
    return np.array([eval_tree(tree, {c: d[c][i] for c in d}) for i in range(n)], dtype=np.float64)


def group_stats(group_cols, values, mask):
    """{key tuple: (sum, min, max, count, sum of |terms|)} of `values` over the docs of `mask`: the sum from 0.0 in doc
    order (numpy float64 adds, no pairwise tree: one doc at a time), min / max in key order (-0.0 below +0.0, NaN on
    top)."""
    out = {}
    idx = np.nonzero(np.asarray(mask))[0]
    gcols = [np.asarray(c)[idx].tolist() for c in group_cols]
    v = np.asarray(values, dtype=np.float64)[idx].tolist()
    for i, x in enumerate(v):
        k = tuple(g[i] for g in gcols)
        s = out.get(k)
        if s is None:
            out[k] = [0.0 + x, x, x, 1, abs(x)]
        else:
            s[0] += x
            s[1] = x if key(x) < key(s[1]) else s[1]
            s[2] = x if key(x) > key(s[2]) else s[2]
            s[3] += 1
            s[4] += abs(x)
    return {k: tuple(s) for k, s in out.items()}


def fused_differs(a, b, c):
    """round(a * b + c) != round(round(a * b) + c), by exact rational arithmetic: a doc on which a fused multiply-add
    would change the bits."""
    F = fractions.Fraction
    exact = F(a) * F(b) + F(c)
    fused = float(exact)  # (Fraction -> float rounds to nearest even, once)
    return bits(fused) != bits(a * b + c)
