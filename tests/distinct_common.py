"""Shared by the DISTINCTCOUNT tests: the reference's recorded answers (tests/golden/kat_inter_distinct.json) and the
yardstick the oracle does not have -- a brute-force set count over numpy columns."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_DISTINCT = json.load(open(os.path.join(HERE, "golden", "kat_inter_distinct.json")))


def json_filter_mask(j, cols, n):
    """kat_sv.json's filter form evaluated over value columns (numpy int64 arrays, lists of str)."""
    if j is None:
        return np.ones(n, dtype=bool)
    if "and" in j:
        return np.logical_and.reduce([json_filter_mask(c, cols, n) for c in j["and"]])
    if "or" in j:
        return np.logical_or.reduce([json_filter_mask(c, cols, n) for c in j["or"]])
    if "not" in j:
        return ~json_filter_mask(j["not"], cols, n)
    col = cols[j["col"]]
    is_str = not isinstance(col, np.ndarray)
    arr = np.array(col) if is_str else col
    conv = (lambda v: v) if is_str else int
    t = j["pred"]
    if t == "EQ":
        return arr == conv(j["value"])
    if t == "NOT_EQ":
        return arr != conv(j["value"])
    if t in ("IN", "NOT_IN"):
        m = np.isin(arr, [conv(v) for v in j["values"]])
        return m if t == "IN" else ~m
    m = np.ones(n, dtype=bool)
    if j["lower"] != "*":
        m &= (arr >= conv(j["lower"])) if j.get("li", True) else (arr > conv(j["lower"]))
    if j["upper"] != "*":
        m &= (arr <= conv(j["upper"])) if j.get("ui", True) else (arr < conv(j["upper"]))
    return m


def distinct_counts(group_cols, value_cols, mask):
    """{key tuple: [number of distinct values of each value column]} over the docs of `mask` (groups without a doc
    absent).  Columns are sequences of equal length; keys and values are compared as Python objects."""
    sets = {}
    idx = np.nonzero(np.asarray(mask))[0].tolist()
    gcols = [np.asarray(c).tolist() for c in group_cols]
    vcols = [np.asarray(c).tolist() for c in value_cols]
    for i in idx:
        key = tuple(g[i] for g in gcols)
        s = sets.get(key)
        if s is None:
            s = sets[key] = [set() for _ in vcols]
        for a, v in enumerate(vcols):
            s[a].add(v[i])
    return {k: [len(x) for x in s] for k, s in sets.items()}
