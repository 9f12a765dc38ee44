"""Cost of conditional aggregation on the C3-shaped table of tools/expr_cost.py (one GPU): the arithmetic sum
SUM(mult(a,b)), the same sum under a condition -- SUM(CASE WHEN c < 2500 THEN a * b ELSE 0 END), half the docs take
each branch -- and the arithmetic predicate a * b > 50000000 as a WHERE leaf, each under C3's selective filter (the
sparse expression instance 12), under the day range alone and with no filter at all (the dense instance 13).  Plans are
warmed, then timed in alternation --repeats times of --steps executions each (PGPU_OPT_TIMING events: the whole
execution and its scan launch).  With PGPU_LIB naming a library from before the conditional ops, the CASE queries are
skipped and the others measure that library's evaluator.  Prints one JSON line.

    python tools/case_cost.py --segments 20 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUMS = {"mult": "SUM(mult(a,b))", "case": "SUM(CASE WHEN c < 2500 THEN a * b ELSE 0 END)"}
FILTERS = {"c3": "daysSinceEpoch BETWEEN 17849 AND 17856 AND accountId IN (123456789)",
           "days": "daysSinceEpoch BETWEEN 17849 AND 17856", "all": ""}
LEAF = "a * b > 50000000"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from pinot_amd import _lib as L
    from pinot_amd.executor import GpuTable
    from pinot_amd.query import parse_query
    from pinot_amd.workloads import account_ids, double_table, zipf_cdf
    n = 100_000
    schema = [("daysSinceEpoch", "INT"), ("accountId", "INT"), ("a", "INT"), ("b", "INT"), ("c", "INT"), ("d", "INT"),
              ("md", "DOUBLE")]
    gen = [{"kind": "UNIFORM", "column_index": 0, "lo": 17532, "hi": 17897},
           {"kind": "ZIPF", "column_index": 1, "cdf": zipf_cdf(n), "ids": account_ids(n)},
           {"kind": "UNIFORM", "column_index": 2, "lo": 0, "hi": 1000},
           {"kind": "UNIFORM", "column_index": 3, "lo": 1, "hi": 100_000},
           {"kind": "UNIFORM", "column_index": 4, "lo": 0, "hi": 5000},
           {"kind": "UNIFORM", "column_index": 5, "lo": 1, "hi": 300},
           {"kind": "TABLE", "column_index": 6, "table": double_table(100_000, 3, -1e6, 1e6)}]
    t = GpuTable(schema)
    hs = [t.generate_segment(gen, row0=i * args.docs, num_docs=args.docs) for i in range(args.segments)]
    sql = {}
    for f, where in FILTERS.items():
        for s, select in SUMS.items():
            sql["%s_%s" % (f, s)] = "SELECT %s, COUNT(*) FROM t%s GROUP BY daysSinceEpoch" % (select, " WHERE " + where if where else "")
        sql["%s_leaf" % f] = "SELECT COUNT(*) FROM t WHERE %s GROUP BY daysSinceEpoch" % (where + " AND " + LEAF if where else LEAF)
    queries = {name: parse_query(s, filter_expressions=True) for name, s in sql.items()}
    for q in queries.values():
        q.timing = True

    def run(name, describe=False):
        with t.plan_execute(hs, queries[name]) as p:
            r = p.finalize()
            total, scan = p.timing_us()[:2]
            if not describe:
                return total, scan
            return r.as_dict(), {"group_path": p.group_path(), "variant": p.scan_geometry()["variant"],
                                 "docs_scanned": r.stats.as_tuple()[0]}

    info, results, skipped = {}, {}, []
    for name in list(queries):
        try:
            for _ in range(args.warmup):
                run(name)
        except L.PinotGpuError as e:  # a library without the conditional ops: "unknown op"
            if "case" not in name:
                raise
            skipped.append(name)
            del queries[name]
            continue
        results[name], info[name] = run(name, describe=True)
    for f in FILTERS:  # the same groups and counts whatever is summed
        if "%s_case" % f in results:
            assert {k: v[1] for k, v in results["%s_case" % f].items()} == {k: v[1] for k, v in results["%s_mult" % f].items()}
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for name in queries:
            runs = [run(name) for _ in range(args.steps)]
            pair[name] = (statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs))
        pairs.append(pair)
    med = {n_: (statistics.median(p[n_][0] for p in pairs), statistics.median(p[n_][1] for p in pairs)) for n_ in queries}
    out = {"tool": "case_cost", "library": os.environ.get("PGPU_LIB", "in-tree"), "queries": sql, "skipped": skipped,
           "segments": args.segments, "docs_per_segment": args.docs, "steps": args.steps, "repeats": args.repeats}
    for name in queries:
        out["execute_us_" + name] = med[name][0]
        out["scan_us_" + name] = med[name][1]
        out["plan_" + name] = info[name]
    for f in FILTERS:
        if "%s_case" % f in med:
            out["scan_ratio_%s_case_to_mult" % f] = med["%s_case" % f][1] / med["%s_mult" % f][1]
    out["pairs_us"] = [{n_: list(p[n_]) for n_ in p} for p in pairs]
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
