"""Cost of DISTINCTCOUNT on the C3 AdAnalytics workload (one GPU): the workload's query with one DISTINCTCOUNT over the
highest-cardinality column whose side bitmap fits the cap (not a group-by or filter column), against the same query
with MAX of that column -- the same column bytes are read, the difference is the bitmap traffic (tested loads, the
atomics of first sightings, the popcount pass) and the scan instance (the DC instance is the general sparse one; the
MAX query takes the pure-AND instance).  Both plans are warmed, then timed in alternation --repeats times of --steps
executions each (PGPU_OPT_TIMING events: the whole execution and its scan launch; their difference holds the
bitmap's memset, the slab fold and distinct_popcount_kernel).  Prints one JSON line.

    python tools/distinct_cost.py --segments 20 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP_BYTES = 1 << 30  # kDistinctMaxBytes (internal.h)


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
    with t.plan(hs, base) as p:
        keys = p.layout()[1]  # the dense key space of the workload's GROUP BY under its filter
    used = set(base.columns())
    col, card = None, 0
    for name, _ in w.schema:
        n = len(t.dictionary(name))
        if name not in used - {c for _, c in base.aggregations} and n >= card and keys * ((n + 63) // 64) * 8 <= CAP_BYTES:
            col, card = name, n
    select = ", ".join("%s(%s)" % a for a in base.aggregations)
    tail = w.sql[w.sql.upper().index(" FROM "):]
    queries = {}
    for fn in ("MAX", "DISTINCTCOUNT"):
        q = parse_query("SELECT %s, %s(%s)%s" % (select, fn, col, tail), num_groups_limit=w.num_groups_limit)
        q.timing = True
        queries[fn] = q

    def run(fn, describe=False):
        with t.plan_execute(hs, queries[fn]) as p:
            r = p.finalize()
            total, scan = p.timing_us()[:2]
            if not describe:
                return total, scan
            return r.as_dict(), {"group_path": p.group_path(), "variant": p.scan_geometry()["variant"],
                                 "keys": p.layout()[1]}

    info, results = {}, {}
    for fn in queries:
        for _ in range(args.warmup):
            run(fn)
        results[fn], info[fn] = run(fn, describe=True)
    # the same groups and sums either way; a group's distinct values are at most its docs' values up to its MAX
    assert set(results["MAX"]) == set(results["DISTINCTCOUNT"])
    for k, a in results["MAX"].items():
        b = results["DISTINCTCOUNT"][k]
        assert a[:-1] == b[:-1] and isinstance(b[-1], int) and 1 <= b[-1] <= card, (k, a, b)
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for fn in queries:
            runs = [run(fn) for _ in range(args.steps)]
            pair[fn] = (statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs))
        pairs.append(pair)
    med = {fn: (statistics.median(p[fn][0] for p in pairs), statistics.median(p[fn][1] for p in pairs)) for fn in queries}
    words = (card + 63) // 64
    print(json.dumps({
        "tool": "distinct_cost", "workload": w.name, "column": col, "cardinality": card,
        "queries": {fn: "SELECT %s, %s(%s)%s" % (select, fn, col, tail) for fn in queries},
        "segments": args.segments, "docs_per_segment": args.docs, "steps": args.steps, "repeats": args.repeats,
        "bitmap_bytes": info["DISTINCTCOUNT"]["keys"] * words * 8, "bitmap_words_per_key": words,
        "execute_us_max": med["MAX"][0], "execute_us_distinctcount": med["DISTINCTCOUNT"][0],
        "scan_us_max": med["MAX"][1], "scan_us_distinctcount": med["DISTINCTCOUNT"][1],
        "scan_ratio": med["DISTINCTCOUNT"][1] / med["MAX"][1],
        "outside_scan_us_max": med["MAX"][0] - med["MAX"][1],
        "outside_scan_us_distinctcount": med["DISTINCTCOUNT"][0] - med["DISTINCTCOUNT"][1],
        "pairs_us": [{fn: list(p[fn]) for fn in p} for p in pairs],
        "plan_max": info["MAX"], "plan_distinctcount": info["DISTINCTCOUNT"],
        "distinct_counts": {str(k[0]): v[-1] for k, v in sorted(results["DISTINCTCOUNT"].items())}}))
    t.close()


if __name__ == "__main__":
    main()
