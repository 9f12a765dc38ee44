"""Cost of an expression leaf in WHERE on the C3-shaped table of tools/expr_cost.py (one GPU): COUNT(*), SUM(md) GROUP BY
daysSinceEpoch under `mult(a,b) > t` alone at about 1 % and 50 % matched and ANDed with C3's filter, each beside the same
query with a plain range leaf of about the same selectivity (a >= 991, a >= 500).  Plans are warmed, then timed in
alternation --repeats times of --steps executions each (PGPU_OPT_TIMING events: the whole execution and its scan
launch).  The expression leaf is evaluated by a kernel of its own in front of the scan, so the time of an execution that
is not its scan launch holds it: `front_us` = execute - scan per query, and the pre-kernel's time is the front of the
expression query less the front of its plain twin (whose leaf is evaluated inside the scan).  Bytes per doc of the
pre-kernel, derived: the operands' forward-index bits (a: 10, b: 17) plus the docbits it writes (4 bytes per 32 docs).
Prints one JSON line.

    python tools/expr_filter_cost.py --segments 20 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C3 = "daysSinceEpoch BETWEEN 17849 AND 17856 AND accountId IN (123456789)"
# P(a * b > t) for a in [0, 1000], b in [1, 100000] uniform: 1 - s + s ln s with s = t / 1e8
WHERE = {"expr_1": "mult(a,b) > 86000000", "plain_1": "a >= 991", "expr_50": "mult(a,b) > 18670000", "plain_50": "a >= 500",
         "c3_expr_1": C3 + " AND mult(a,b) > 86000000", "c3_plain_1": C3 + " AND a >= 991",
         "c3_expr_50": C3 + " AND mult(a,b) > 18670000", "c3_plain_50": C3 + " AND a >= 500"}
HBM_MEASURED_TB_S = 6.29  # a float4 copy on this part; 8.0 by specification


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
    for name, where in WHERE.items():
        sql[name] = "SELECT COUNT(*), SUM(md) FROM t WHERE %s GROUP BY daysSinceEpoch" % where
        queries[name] = parse_query(sql[name], filter_expressions=True)
        queries[name].timing = True

    def run(name, describe=False):
        with t.plan_execute(hs, queries[name]) as p:
            r = p.finalize()
            total, scan = p.timing_us()[:2]
            if not describe:
                return total, scan
            return {"group_path": p.group_path(), "variant": p.scan_geometry()["variant"], "stats": list(r.stats.as_tuple())}

    info = {}
    for name in queries:
        for _ in range(args.warmup):
            run(name)
        info[name] = run(name, describe=True)
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for name in queries:
            runs = [run(name) for _ in range(args.steps)]
            pair[name] = (statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs))
        pairs.append(pair)
    med = {q: (statistics.median(p[q][0] for p in pairs), statistics.median(p[q][1] for p in pairs)) for q in queries}
    docs = args.segments * args.docs
    floor_bytes = (10 + 17) / 8.0 + 4.0 / 32.0
    out = {"tool": "expr_filter_cost", "queries": sql, "segments": args.segments, "docs_per_segment": args.docs,
           "steps": args.steps, "repeats": args.repeats, "pre_kernel_bytes_per_doc_floor": floor_bytes,
           "hbm_measured_tb_s": HBM_MEASURED_TB_S}
    for name in queries:
        out["execute_us_" + name] = med[name][0]
        out["scan_us_" + name] = med[name][1]
        out["front_us_" + name] = med[name][0] - med[name][1]
        out["plan_" + name] = info[name]
        out["matched_fraction_" + name] = info[name]["stats"][0] / docs
    for k in ("1", "50", ):
        for pre in ("", "c3_"):
            e, p = "%sexpr_%s" % (pre, k), "%splain_%s" % (pre, k)
            pk = out["front_us_" + e] - out["front_us_" + p]
            out["pre_kernel_us_" + e] = pk
            out["execute_ratio_" + e] = med[e][0] / med[p][0]
            if pk > 0:
                out["pre_kernel_floor_tb_s_" + e] = docs * floor_bytes / (pk * 1e-6) / 1e12
                out["pre_kernel_share_of_hbm_" + e] = docs * floor_bytes / (pk * 1e-6) / 1e12 / HBM_MEASURED_TB_S
    out["pairs_us"] = [{q: list(p[q]) for q in p} for p in pairs]
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
