"""Cost of bit-reproducible FLOAT / DOUBLE sums (query option exact_fp_sum, PGPU_OPT_EXACT_FP_SUM) on the C2
workload at its BASELINE shape (100 segments of 1 M docs on one GPU): the scan kernel's time (PGPU_OPT_TIMING events)
of the workload's query with and without the option, both plans warmed, then timed in alternation --repeats times of
--steps executions each, so that whatever else shares the GPU touches both alike.  Prints one JSON line: the medians,
every repeat's pair, the ratio of the medians, the spread of each side over its repeats, and the plan's {mode, E, K, W}.

    python tools/fp_sum_cost.py --segments 100 --docs 1000000
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--segments", type=int, default=100)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from pinot_amd.executor import GpuTable
    from pinot_amd.query import parse_query
    from pinot_amd.workloads import WORKLOADS
    w = WORKLOADS[args.workload]()
    t = GpuTable(w.schema)
    hs = [t.generate_segment(w.gen, row0=i * args.docs, num_docs=args.docs) for i in range(args.segments)]
    queries = {}
    for exact in (False, True):
        q = parse_query(w.sql, num_groups_limit=w.num_groups_limit, exact_fp_sum=exact)
        q.timing = True
        queries[exact] = q

    def scan_us(exact, describe=False):
        with t.plan_execute(hs, queries[exact]) as p:
            r = p.finalize()
            us = p.timing_us()[1]
            if not describe:
                return us
            na = len(queries[exact].aggregations)
            return r.as_dict(), {"group_path": p.group_path(), "variant": p.scan_geometry()["variant"],
                                 "formats": [p.fp_sum_format(a) for a in range(na)]}

    info = {}
    results = {}
    for exact in (False, True):
        for _ in range(args.warmup):
            scan_us(exact)
        results[exact], info[exact] = scan_us(exact, describe=True)
    # same groups and integer aggregations; the double sums within the oracle's 1e-9
    assert set(results[False]) == set(results[True])
    for k, a in results[False].items():
        for x, y in zip(a, results[True][k]):
            assert x == y or abs(x - y) <= 1e-9 * max(abs(x), abs(y)), (k, x, y)
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for exact in (False, True):
            pair[exact] = statistics.median(scan_us(exact) for _ in range(args.steps))
        pairs.append((pair[False], pair[True]))
    plain = [a for a, _ in pairs]
    exact = [b for _, b in pairs]
    fm = [f for f in info[True]["formats"] if f["mode"] != "none"]
    print(json.dumps({
        "tool": "fp_sum_cost", "workload": w.name, "query": w.sql, "segments": args.segments,
        "docs_per_segment": args.docs, "steps": args.steps, "repeats": args.repeats,
        "scan_us_plain": statistics.median(plain), "scan_us_exact_fp_sum": statistics.median(exact),
        "ratio": statistics.median(exact) / statistics.median(plain),
        "spread_plain": (max(plain) - min(plain)) / statistics.median(plain),
        "spread_exact_fp_sum": (max(exact) - min(exact)) / statistics.median(exact),
        "pairs_us": pairs, "plan_plain": info[False], "plan_exact_fp_sum": info[True],
        "fp_sum_format": fm[0] if fm else None}))
    t.close()


if __name__ == "__main__":
    main()
