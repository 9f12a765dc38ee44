"""Shared by the PERCENTILE tests: the reference's recorded answers (tests/golden/kat_inter_percentile.json) and the
yardstick the oracle does not have -- a numpy sort per group, indexed by PercentileAggregationFunction's formula."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_PERCENTILE = json.load(open(os.path.join(HERE, "golden", "kat_inter_percentile.json")))


def java_index(size, p):
    """PercentileAggregationFunction.extractFinalResult (:152-165): size - 1 for the 100th percentile, else
    (int)((double)size * percentile / 100.0) -- Python floats are IEEE doubles and evaluate left to right as Java does."""
    if p == 100:
        return size - 1
    return int(float(size) * float(p) / 100.0)


def percentiles(group_cols, value_col, mask, p):
    """{key tuple: the value at the percentile's index of the group's sorted values, as a float} over the docs of
    `mask` (groups without a doc absent).  (double)value of an integer column, as getDoubleValuesSV converts it."""
    mask = np.asarray(mask)
    v = np.asarray(value_col)[mask]
    gcols = [np.asarray(c)[mask].tolist() for c in group_cols]
    groups = {}
    for i in range(len(v)):
        groups.setdefault(tuple(g[i] for g in gcols), []).append(i)
    out = {}
    for k, idx in groups.items():
        s = np.sort(v[idx])
        out[k] = float(s[java_index(len(s), p)])
    return out
