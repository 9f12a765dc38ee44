"""Cost of expressions inside aggregations on a C3-shaped table (one GPU): AdAnalytics' daysSinceEpoch / accountId with
four INT columns a, b, c, d and a DOUBLE column md, and three sums over it -- SUM(md), a plain DOUBLE column;
SUM(mult(a,b)); SUM(add(div(a,b),div(c,d))) -- each under C3's selective filter (0.18 % of the docs: every instance is
the sparse shape, instance 12 for an expression), under the day range alone (2 %) and with no filter at all, where
SUM(md) takes the whole-group (dense) instance 1 and an expression plan instance 13 -- and, for the comparison of the
two expression instances on the same scan, the unfiltered queries once more with dense_selectivity raised so that
they run the sparse instances.  Two sums over the math ops ride along, SUM(floor(a / 10)) and SUM(mod(a, 7)); with PGPU_LIB
naming a library from before those ops they are skipped and the others measure that library's evaluator.  Plans are
warmed, then timed in
alternation --repeats times of --steps executions each (PGPU_OPT_TIMING events: the whole execution and its scan
launch).  Bytes per matched doc are what the forms gather: per operand a dictId (4-byte window of the forward index)
and its 8-byte double.  Prints one JSON line.

    python tools/expr_cost.py --segments 20 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUMS = {"md": "SUM(md)", "mult": "SUM(mult(a,b))", "add_div_div": "SUM(add(div(a,b),div(c,d)))",
        "floor_div": "SUM(floor(a / 10))", "mod": "SUM(mod(a, 7))"}
OPERANDS = {"md": 1, "mult": 2, "add_div_div": 4, "floor_div": 1, "mod": 1}
NEW = ("floor_div", "mod")  # (the ops a parent library answers "unknown op" to)
FILTERS = {"c3": " WHERE daysSinceEpoch BETWEEN 17849 AND 17856 AND accountId IN (123456789)",
           "days": " WHERE daysSinceEpoch BETWEEN 17849 AND 17856", "all": "", "all_sparse": ""}
CONFIG = {"all_sparse": {"dense_selectivity": 2.0}}  # (no plan's estimate reaches it: the sparse instances)


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
    sql, queries = {}, {}
    for f, where in FILTERS.items():
        for s, select in SUMS.items():
            name = "%s_%s" % (f, s)
            sql[name] = "SELECT %s, COUNT(*) FROM t%s GROUP BY daysSinceEpoch" % (select, where)
            queries[name] = parse_query(sql[name])
            queries[name].timing = True

    current = [None]

    def run(name, describe=False):
        f = name[:-len("_" + max((s for s in SUMS if name.endswith("_" + s)), key=len))]
        if current[0] != f:  # (a change of settings clears the plan cache: once per block of runs)
            t.reset_config()
            if f in CONFIG:
                t.set_config(**CONFIG[f])
            current[0] = f
        with t.plan_execute(hs, queries[name]) as p:
            r = p.finalize()
            total, scan = p.timing_us()[:2]
            if not describe:
                return total, scan
            return r.as_dict(), {"group_path": p.group_path(), "variant": p.scan_geometry()["variant"],
                                 "docs_scanned": r.stats.as_tuple()[0], "entries_post_filter": r.stats.as_tuple()[2]}

    info, results, skipped = {}, {}, []
    for name in list(queries):
        try:
            for _ in range(args.warmup):
                run(name)
        except L.PinotGpuError:  # a library without the math ops: "unknown op"
            if not name.endswith(tuple("_" + s for s in NEW)):
                raise
            skipped.append(name)
            del queries[name]
            continue
        results[name], info[name] = run(name, describe=True)
    for f in FILTERS:  # the same groups and counts whatever is summed
        counts = [{k: v[1] for k, v in results["%s_%s" % (f, s)].items()} for s in SUMS if "%s_%s" % (f, s) in results]
        assert all(c == counts[0] for c in counts)
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for name in queries:
            runs = [run(name) for _ in range(args.steps)]
            pair[name] = (statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs))
        pairs.append(pair)
    med = {n_: (statistics.median(p[n_][0] for p in pairs), statistics.median(p[n_][1] for p in pairs)) for n_ in queries}
    out = {"tool": "expr_cost", "library": os.environ.get("PGPU_LIB", "in-tree"), "queries": sql, "skipped": skipped,
           "segments": args.segments, "docs_per_segment": args.docs,
           "steps": args.steps, "repeats": args.repeats,
           "gathered_bytes_per_matched_doc": {s: 12 * k for s, k in OPERANDS.items()}}
    for name in queries:
        out["execute_us_" + name] = med[name][0]
        out["scan_us_" + name] = med[name][1]
        out["plan_" + name] = info[name]
    for f in FILTERS:
        for s in SUMS:
            if s != "md" and "%s_%s" % (f, s) in med:
                out["scan_ratio_%s_%s" % (f, s)] = med["%s_%s" % (f, s)][1] / med["%s_md" % f][1]
    out["pairs_us"] = [{n_: list(p[n_]) for n_ in p} for p in pairs]
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
