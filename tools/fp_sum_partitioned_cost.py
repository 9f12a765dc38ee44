"""Cost and benefit of fixed-point FLOAT / DOUBLE sums on the partitioned group-by, on a C5-shaped query: the C5 key
space (k1 x k2 x k3 = 10^7 dense keys) with a DOUBLE column from a PGPU_GEN_TABLE generator (C2's `md` values) summed,
SELECT SUM(md), COUNT(*) FROM t GROUP BY k1, k2, k3, over --segments segments of --docs docs on one GPU.  Three plans:

  agreed     exact_fp_sum with agreed ranges (the table's own): the radix-partitioned pipeline, K8d's FX instance;
  plain      exact_fp_sum through pgpu_plan_create_execute: the scan kernel's global table (where such a query ran
             before agreed plans existed);
  float64    without the option: the radix-partitioned pipeline with float64 LDS atomics.

Each plan is warmed, then the three are timed in alternation --repeats times of --steps executions each (PGPU_OPT_TIMING
events: the whole execute and the scan / partition launches).  The agreed and the plain plan must give the same bits;
the float64 plan's sums agree within 1e-9.  Prints one JSON line.  --only NAME --steps N: N executions of one plan and
nothing else (the run a kernel profiler wraps).

    python tools/fp_sum_partitioned_cost.py --segments 16 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SQL = "SELECT SUM(md), COUNT(*) FROM t GROUP BY k1, k2, k3"
PLANS = ("agreed", "plain", "float64")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=16)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=PLANS)
    args = ap.parse_args()
    from pinot_amd.executor import GpuTable
    from pinot_amd.query import parse_query
    from pinot_amd.workloads import double_table
    schema = [("k1", "INT"), ("k2", "INT"), ("k3", "INT"), ("md", "DOUBLE")]
    gen = [{"kind": "UNIFORM", "column_index": 0, "lo": 0, "hi": 1000},
           {"kind": "UNIFORM", "column_index": 1, "lo": 0, "hi": 100},
           {"kind": "UNIFORM", "column_index": 2, "lo": 0, "hi": 100},
           {"kind": "TABLE", "column_index": 3, "table": double_table(100_000, 3, -1e6, 1e6)}]
    t = GpuTable(schema)
    hs = [t.generate_segment(gen, row0=i * args.docs, num_docs=args.docs) for i in range(args.segments)]
    queries = {}
    for name in PLANS:
        q = parse_query(SQL, num_groups_limit=1_000_000_000, exact_fp_sum=name != "float64")
        q.timing = True
        queries[name] = q
    ranges = t.fp_sum_ranges(hs, queries["agreed"])

    def run(name, describe=False):
        with t.plan_execute(hs, queries[name], fp_sum_ranges=ranges if name == "agreed" else None) as p:
            r = p.finalize()
            tm = p.timing_us()
            if not describe:
                return tm[0], tm[1]
            return r, {"group_path": p.group_path(), "format": p.fp_sum_format(0), "slots": p.layout()[0],
                       "groups": len(r)}

    if args.only:
        for _ in range(args.steps):
            run(args.only)
        t.close()
        return
    info, sums = {}, {}
    for name in PLANS:
        for _ in range(args.warmup):
            run(name)
        r, info[name] = run(name, describe=True)
        sums[name] = (r.gids, r._col[2][0][1].copy())
    import numpy as np
    for name in ("plain", "float64"):  # hash-free dense results: the groups come in key order on every path
        assert np.array_equal(sums[name][0], sums["agreed"][0]), name
    assert np.array_equal(sums["agreed"][1].view(np.int64), sums["plain"][1].view(np.int64)), "paths differ in bits"
    a, f = sums["agreed"][1], sums["float64"][1]
    assert np.all(np.abs(a - f) <= 1e-9 * np.maximum(np.maximum(np.abs(a), np.abs(f)), 1e6)), "float64 plan off"
    reps = []
    for _ in range(args.repeats):
        rep = {}
        for name in PLANS:
            ts = [run(name) for _ in range(args.steps)]
            rep[name] = (statistics.median(x[0] for x in ts), statistics.median(x[1] for x in ts))
        reps.append(rep)
    out = {"tool": "fp_sum_partitioned_cost", "query": SQL, "segments": args.segments, "docs_per_segment": args.docs,
           "steps": args.steps, "repeats": args.repeats, "plans": info}
    for name in PLANS:
        ex = [r[name][0] for r in reps]
        sc = [r[name][1] for r in reps]
        out[name] = {"execute_us": statistics.median(ex), "launches_us": statistics.median(sc),
                     "execute_us_repeats": ex, "spread": (max(ex) - min(ex)) / statistics.median(ex)}
    out["agreed_over_plain"] = out["agreed"]["execute_us"] / out["plain"]["execute_us"]
    out["agreed_over_float64"] = out["agreed"]["execute_us"] / out["float64"]["execute_us"]
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
