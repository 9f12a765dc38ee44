"""Yardstick of the math and time functions in expressions (tests/test_time_expr_cpu.py, tests/test_time_expr_gpu.py): a
pure-Python interpreter of an emitted program -- Python floats are IEEE doubles, math.fmod is C's fmod, and the long
division is Python's exact integers truncated toward zero -- and the same in typed numpy over whole columns."""
import json
import math
import os
import struct

import numpy as np

from pinot_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_datetime_convert.json")
NAN_KEY = 0x7ff8000000000000


def load_kat():
    with open(GOLDEN) as f:
        return json.load(f)


def bits(d):
    return struct.unpack("<q", struct.pack("<d", float(d)))[0]


def key(d):
    """Double.doubleToLongBits' order as a signed integer (expr_value_key)."""
    if d != d:
        return NAN_KEY
    b = bits(d)
    return b if b >= 0 else b ^ 0x7fffffffffffffff


def tdiv(a, b):
    """Java's long division: truncated toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _unary(op, x):
    if op == L.EXPR_ABS:
        return abs(x)
    if op == L.EXPR_SQRT:
        return math.sqrt(x) if x >= 0 else (x if x == 0 else float("nan"))  # (-0.0 >= 0: sqrt(-0.0) is -0.0)
    if x != x or x in (float("inf"), float("-inf")):
        return x
    r = float(math.ceil(x) if op == L.EXPR_CEIL else math.floor(x))
    return math.copysign(r, x) if r == 0 else r  # ceil(-0.5) is -0.0, floor(-0.0) is -0.0


def _mod(a, b):
    if a != a or b != b or b == 0 or a in (float("inf"), float("-inf")):
        return float("nan")
    return math.fmod(a, b)


def run_program(ops, row):
    """The value of program `ops` ((op, column name, literal) triples) over row: {column name: number}."""
    st = []
    for op, col, lit in ops:
        if op == L.EXPR_COLUMN:
            st.append(float(row[col]))
        elif op == L.EXPR_LITERAL:
            st.append(float(lit))
        elif L.EXPR_ABS <= op <= L.EXPR_SQRT:
            st.append(_unary(op, st.pop()))
        elif op == L.EXPR_SELECT:
            cond, then, els = st.pop(), st.pop(), st.pop()
            st.append(then if cond != 0.0 else els)
        else:
            b, a = st.pop(), st.pop()
            if op == L.EXPR_ADD:
                st.append(a + b)
            elif op == L.EXPR_SUB:
                st.append(a - b)
            elif op == L.EXPR_MULT:
                st.append(a * b)
            elif op == L.EXPR_DIV:
                st.append(a / b if b != 0 else (float("nan") if a == 0 or a != a else math.copysign(float("inf"), a) * math.copysign(1.0, b)))
            elif op == L.EXPR_MOD:
                st.append(_mod(a, b))
            elif op == L.EXPR_LDIV:
                assert a == int(a) and b == int(b) and abs(a) <= 2 ** 53 and 1 <= b <= 2 ** 53
                st.append(float(tdiv(int(a), int(b))))
            elif op in (L.EXPR_AND, L.EXPR_OR):
                st.append(min(a, b) if op == L.EXPR_AND else max(a, b))
            else:
                ka, kb = key(a), key(b)
                st.append(1.0 if {L.EXPR_EQ: ka == kb, L.EXPR_NE: ka != kb, L.EXPR_GT: ka > kb, L.EXPR_GE: ka >= kb,
                                  L.EXPR_LT: ka < kb, L.EXPR_LE: ka <= kb}[op] else 0.0)
    assert len(st) == 1
    return st[0]


def np_tdiv(a, n):
    """int64 a / n truncated toward zero, which numpy's // is not."""
    a = np.asarray(a, dtype=np.int64)
    q = np.abs(a) // np.int64(n)
    return np.where(a < 0, -q, q).astype(np.int64)


def np_datetimeconvert(v, n, to_ms, g, from_ms, m):
    """EpochToEpochTransformer over int64 v: to_ms / from_ms are ('mult' | 'ldiv', k)."""
    v = np.asarray(v, dtype=np.int64) * np.int64(n)
    v = v * np.int64(to_ms[1]) if to_ms[0] == "mult" else np_tdiv(v, to_ms[1])
    v = np_tdiv(v, g) * np.int64(g)
    v = v * np.int64(from_ms[1]) if from_ms[0] == "mult" else np_tdiv(v, from_ms[1])
    return np_tdiv(v, m)
