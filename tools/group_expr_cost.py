"""Cost of expressions in GROUP BY on a C3-shaped table (one GPU): AdAnalytics' daysSinceEpoch / accountId with the INT
columns a (1000 values), p and s (30 and 29 values), and two real columns of the derived columns' cardinality and bit
width -- r3 (3 values, 2 bits) beside the one-operand CASE over a, rp beside the two-operand product p * s.

  build   the one-off cost per segment of each derived column, from the library's own event pairs (PGPU_TRACE=derive: the
          candidates, ids and pack kernels and the whole build with its host steps), the HBM bytes it keeps, and the ids
          kernel's achieved bandwidth against the bytes it must move: the operands' forward-index words in, 4 bytes per
          doc out.
  query   GROUP BY <expression> against GROUP BY the real column, under C3's selective filter and with no filter.  The
          pair must report the same scan instance, group-table path and geometry (asserted: the derived column is an
          ordinary dictionary column to the scan); the times are recorded.  Plans are warmed, then timed in alternation
          --repeats times of --steps executions each (PGPU_OPT_TIMING events: the whole execution and its scan launch).

A time bucket rides along: GROUP BY datetimeconvert(ts, milliseconds -> hours) over a LONG column of milliseconds spanning 48 hours beside
the real column rh of its 48 values; with PGPU_LIB naming a library from before the time ops it is skipped.

Prints one JSON line.

    python tools/group_expr_cost.py --segments 20 --docs 1000000
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["PGPU_TRACE"] = ",".join(filter(None, [os.environ.get("PGPU_TRACE"), "derive"]))  # before the library loads

CASE = "CASE WHEN a < 180 THEN 0 WHEN a < 650 THEN 1 ELSE 2 END"
HOURS = "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')"
KEYS = {"case": CASE, "real3": "r3", "prod": "p * s", "realp": "rp", "hours": HOURS, "realh": "rh"}
PAIRS = {"case": "real3", "prod": "realp", "hours": "realh"}
OPERAND_COLUMNS = {"case": ["a"], "prod": ["p", "s"], "hours": ["ts"]}
NEW = ("hours",)  # (the ops a parent library answers "unknown op" to)
FILTERS = {"c3": " WHERE daysSinceEpoch BETWEEN 17849 AND 17856 AND accountId IN (123456789)", "all": ""}
TRACE = re.compile(r"\[pgpu\] derive (\S+) segment (\d+) docs (\d+) candidates (\d+) unique (\d+) card (\d+) bits (\d+) "
                   r"fwd_bytes (\d+): candidates_us ([\d.]+) ids_us ([\d.]+) pack_us ([\d.]+) build_us ([\d.]+)")


class CaptureStderr:
    """The process's stderr (the library writes to fd 2) into a file while the block runs."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", errors="replace")
        self.tmp.close()


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
    from pinot_amd.workloads import account_ids, zipf_cdf
    n = 100_000
    products = len({x * y for x in range(30) for y in range(1, 30)})
    schema = [("daysSinceEpoch", "INT"), ("accountId", "INT"), ("a", "INT"), ("p", "INT"), ("s", "INT"), ("r3", "INT"),
              ("rp", "INT"), ("ts", "LONG"), ("rh", "INT")]
    gen = [{"kind": "UNIFORM", "column_index": 0, "lo": 17532, "hi": 17897},
           {"kind": "ZIPF", "column_index": 1, "cdf": zipf_cdf(n), "ids": account_ids(n)},
           {"kind": "UNIFORM", "column_index": 2, "lo": 0, "hi": 1000},
           {"kind": "UNIFORM", "column_index": 3, "lo": 0, "hi": 30},
           {"kind": "UNIFORM", "column_index": 4, "lo": 1, "hi": 30},
           {"kind": "UNIFORM", "column_index": 5, "lo": 0, "hi": 3},
           {"kind": "UNIFORM", "column_index": 6, "lo": 0, "hi": products},
           # milliseconds over 48 hours from 2017-09-20T00:00Z: nearly every doc its own value, 48 one-hour buckets
           {"kind": "UNIFORM", "column_index": 7, "lo": 1505865600000, "hi": 1505865600000 + 48 * 3600000},
           {"kind": "UNIFORM", "column_index": 8, "lo": 0, "hi": 48}]
    t = GpuTable(schema)
    hs = [t.generate_segment(gen, row0=i * args.docs, num_docs=args.docs) for i in range(args.segments)]
    sql, queries = {}, {}
    for f, where in FILTERS.items():
        for k, key in KEYS.items():
            name = "%s_%s" % (f, k)
            sql[name] = "SELECT COUNT(*), SUM(a) FROM t%s GROUP BY %s" % (where, key)
            queries[name] = parse_query(sql[name], group_by_expressions=True)
            queries[name].timing = True

    # ---- build: the first plan that names an expression builds its derived column in every segment
    out = {"tool": "group_expr_cost", "library": os.environ.get("PGPU_LIB", "in-tree"), "queries": sql, "segments": args.segments, "docs_per_segment": args.docs,
           "steps": args.steps, "repeats": args.repeats}
    bits_of = {c: t.segment_column_bytes(hs[0], c)[1] for c in ("a", "p", "s", "r3", "rp", "ts")}
    skipped = []
    for k in list(PAIRS):
        before = t.device_bytes()
        try:
            with CaptureStderr() as cap:
                with t.plan(hs, queries["all_" + k]):
                    pass
        except L.PinotGpuError:  # a library without the time ops: "unknown op"
            if k not in NEW:
                raise
            for f in FILTERS:
                for name in ("%s_%s" % (f, k), "%s_%s" % (f, PAIRS[k])):
                    skipped.append(name)
                    del queries[name]
            del PAIRS[k]
            continue
        lines = [m.groups() for m in map(TRACE.search, cap.text.split("\n")) if m]
        assert len(lines) == args.segments, cap.text[-2000:]
        med = lambda i: statistics.median(float(x[i]) for x in lines)  # noqa: E731
        docs, cand, card, bits, fwd_bytes = int(lines[0][2]), int(lines[0][3]), int(lines[0][5]), int(lines[0][6]), int(lines[0][7])
        moved = docs * sum(bits_of[c] for c in OPERAND_COLUMNS[k]) / 8 + 4 * docs
        out["build_" + k] = {
            "expression": KEYS[k], "candidates": cand, "cardinality": card, "bits": bits,
            "forward_index_bytes_per_segment": fwd_bytes,
            "device_bytes_per_segment": (t.device_bytes() - before) / args.segments,  # with the LUT and the operands' values
            "candidates_kernel_us": med(8), "ids_kernel_us": med(9), "pack_kernel_us": med(10), "build_us": med(11),
            "ids_bytes_moved": moved, "ids_gb_per_s": moved / med(9) / 1e3 if med(9) else None}
        assert (card, bits) == tuple(t.segment_column_bytes(hs[0], KEYS[PAIRS[k]])[:2]), "the real column's cardinality and bits"

    out["skipped"] = skipped

    # ---- query
    def run(name, describe=False):
        with t.plan_execute(hs, queries[name]) as p:
            r = p.finalize()
            total, scan = p.timing_us()[:2]
            if not describe:
                return total, scan
            g = p.scan_geometry()
            return r, {"group_path": p.group_path(), "variant": g["variant"], "grid": g["grid"], "lds_bytes": g["lds_bytes"],
                       "tiles": g["tiles"], "tile_chunks": g["tile_chunks"], "docs_scanned": r.stats.as_tuple()[0],
                       "entries_post_filter": r.stats.as_tuple()[2], "groups": len(r)}

    info = {}
    for name in queries:
        for _ in range(args.warmup):
            run(name)
        info[name] = run(name, describe=True)[1]
    for f in FILTERS:  # the condition: the scan cannot tell the derived column from the real one
        for k, real in PAIRS.items():
            a, b = info["%s_%s" % (f, k)], info["%s_%s" % (f, real)]
            # (numEntriesScannedPostFilter differs by design: it counts the expression's operands, not the derived column)
            same = ("group_path", "variant", "grid", "lds_bytes", "tiles", "tile_chunks", "docs_scanned", "groups")
            assert all(a[x] == b[x] for x in same), (f, k, a, b)
    pairs = []
    for _ in range(args.repeats):
        pair = {}
        for name in queries:
            runs = [run(name) for _ in range(args.steps)]
            pair[name] = (statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs))
        pairs.append(pair)
    med = {n_: (statistics.median(p[n_][0] for p in pairs), statistics.median(p[n_][1] for p in pairs)) for n_ in queries}
    for name in queries:
        out["execute_us_" + name] = med[name][0]
        out["scan_us_" + name] = med[name][1]
        out["plan_" + name] = info[name]
    for f in FILTERS:
        for k, real in PAIRS.items():
            out["scan_ratio_%s_%s" % (f, k)] = med["%s_%s" % (f, k)][1] / med["%s_%s" % (f, real)][1]
            out["execute_ratio_%s_%s" % (f, k)] = med["%s_%s" % (f, k)][0] / med["%s_%s" % (f, real)][0]
    out["pairs_us"] = [{n_: list(p[n_]) for n_ in p} for p in pairs]
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
