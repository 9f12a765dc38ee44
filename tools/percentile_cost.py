"""Cost of PERCENTILE on the C3 AdAnalytics workload (one GPU): the workload's query with PERCENTILE50 / 95 / 99 of
impressions (three rows over one side histogram) against the same query with MAX(impressions) -- the same column bytes
are read; the difference is the histogram traffic (one atomic add per matched doc, the memset of the histogram, the
selection kernel) and the scan instance (the histogram instance is the general sparse one; the MAX query takes the
pure-AND instance).  Both plans are warmed, then timed in alternation --repeats times of --steps executions each
(PGPU_OPT_TIMING events: the whole execution and its scan launch; their difference holds the histogram's memset, the
slab fold and percentile_select_kernel).  A second pair measures contention: an unfiltered aggregation-only
PERCENTILE50 over the table's lowest-cardinality column (every doc's add lands on a few hundred cells of one row)
against SUM of that column, which scans the same bytes.  Prints one JSON line.

    python tools/percentile_cost.py --segments 20 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMN = "impressions"
PERCENTILES = (50, 95, 99)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from pinot_amd.executor import GpuTable
    from pinot_amd.query import parse_query
    from pinot_amd.workloads import WORKLOADS
    w = WORKLOADS["adanalytics"]()
    t = GpuTable(w.schema)
    hs = [t.generate_segment(w.gen, row0=i * args.docs, num_docs=args.docs) for i in range(args.segments)]
    base = parse_query(w.sql, num_groups_limit=w.num_groups_limit)
    select = ", ".join("%s(%s)" % a for a in base.aggregations)
    tail = w.sql[w.sql.upper().index(" FROM "):]
    card = len(t.dictionary(COLUMN))
    low, low_card = min(((name, len(t.dictionary(name))) for name, _ in w.schema), key=lambda x: x[1])
    sql = {"MAX": "SELECT %s, MAX(%s)%s" % (select, COLUMN, tail),
           "PERCENTILE": "SELECT %s, %s%s" % (select, ", ".join("PERCENTILE%d(%s)" % (p, COLUMN) for p in PERCENTILES), tail),
           "ONLY_SUM": "SELECT SUM(%s) FROM t" % low,
           "ONLY_PERCENTILE": "SELECT PERCENTILE50(%s) FROM t" % low}
    queries = {}
    for name, s in sql.items():
        q = parse_query(s, num_groups_limit=w.num_groups_limit)
        q.timing = True
        queries[name] = q

    def run(name, describe=False):
        with t.plan_execute(hs, queries[name]) as p:
            r = p.finalize()
            total, scan = p.timing_us()[:2]
            if not describe:
                return total, scan
            return r.as_dict(), {"group_path": p.group_path(), "variant": p.scan_geometry()["variant"],
                                 "keys": p.layout()[1] if queries[name].group_by else 1,
                                 "docs_scanned": r.stats.as_tuple()[0]}

    info, results = {}, {}
    for name in queries:
        for _ in range(args.warmup):
            run(name)
        results[name], info[name] = run(name, describe=True)
    # the same groups and sums either way; a group's percentiles ascend and stay at or below its MAX
    na = len(base.aggregations)
    assert set(results["MAX"]) == set(results["PERCENTILE"])
    for k, a in results["MAX"].items():
        b = results["PERCENTILE"][k]
        assert a[:na] == b[:na] and b[na] <= b[na + 1] <= b[na + 2] <= a[na], (k, a, b)
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for name in queries:
            runs = [run(name) for _ in range(args.steps)]
            pair[name] = (statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs))
        pairs.append(pair)
    med = {n: (statistics.median(p[n][0] for p in pairs), statistics.median(p[n][1] for p in pairs)) for n in queries}
    stride = (card + 3) & ~3
    out = {"tool": "percentile_cost", "workload": w.name, "column": COLUMN, "cardinality": card, "queries": sql,
           "segments": args.segments, "docs_per_segment": args.docs, "steps": args.steps, "repeats": args.repeats,
           "histogram_bytes": info["PERCENTILE"]["keys"] * stride * 4, "histogram_cells_per_key": stride,
           "low_cardinality_column": low, "low_cardinality": low_card}
    for name in queries:
        key = name.lower()
        out["execute_us_" + key] = med[name][0]
        out["scan_us_" + key] = med[name][1]
        out["outside_scan_us_" + key] = med[name][0] - med[name][1]
        out["plan_" + key] = info[name]
    out["scan_ratio"] = med["PERCENTILE"][1] / med["MAX"][1]
    out["only_scan_ratio"] = med["ONLY_PERCENTILE"][1] / med["ONLY_SUM"][1]
    out["pairs_us"] = [{n: list(p[n]) for n in p} for p in pairs]
    out["percentiles"] = {str(k[0]): v[na:] for k, v in sorted(results["PERCENTILE"].items())}
    out["only_percentile"] = results["ONLY_PERCENTILE"][()]
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
