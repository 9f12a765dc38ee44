"""Cost of REGEXP_LIKE on one GPU: a table with a 1 M-value STRING dictionary of URL-like values over 20 segments of 1 M
docs (each segment's dictionary three quarters of the global one, so its local-to-global LUT is a real one), and
`SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(url, 'p') GROUP BY g` for a prefix pattern, an infix pattern and a pattern of
about 200 DFA states.  Per pattern: (a) plan creation (plan cache off: the pattern compiled, the DFA run over the
dictionary, the local sets built and read back, the segments translated) and the first execution, wall clock; (b) the
same for the equivalent IN of the matching values -- the comparison point, which also runs on a library without the
predicate (--in-only); (c) the two kernels' times from HIP events (PGPU_TRACE=regex, one line per plan creation on
stderr); (d) the DFA kernel's achieved bytes per second against the dictionary's device bytes; and the steady execution
of both plans from PGPU_OPT_TIMING.  Prints one JSON line.

    python tools/regexp_cost.py > profiles/regexp_cost.json
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERNS = {
    "prefix": "^/shop/01",
    "infix": "cat-1[0-4]/",
    "states200": "(" + "|".join("/%03d/cat-%02d/" % (7 * i % 100, 13 * i % 100) for i in range(20)) + ")",
}


def _be32(a):
    import numpy as np
    return np.asarray(a, dtype=">i4").tobytes()


def _pack20(ids):
    """Pinot's MSB-first fixed-bit forward index at 20 bits per value (an even number of values: 5 bytes a pair)."""
    import numpy as np
    x = (ids[0::2].astype(np.uint64) << np.uint64(20)) | ids[1::2].astype(np.uint64)
    out = np.empty((len(x), 5), dtype=np.uint8)
    for k in range(5):
        out[:, k] = (x >> np.uint64(32 - 8 * k)) & np.uint64(255)
    return out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--in-only", action="store_true", help="the IN forms alone (a library without REGEXP_LIKE)")
    args = ap.parse_args()
    assert args.docs % 2 == 0
    trace = tempfile.NamedTemporaryFile(mode="r", suffix=".log")
    os.environ["PGPU_TRACE"] = ",".join(x for x in (os.environ.get("PGPU_TRACE"), "regex") if x)
    saved = os.dup(2)
    os.dup2(os.open(trace.name, os.O_WRONLY), 2)  # the library's trace lines, read back below
    try:
        run(args, trace)
    except BaseException:
        os.dup2(saved, 2)
        trace.seek(0)
        sys.stderr.write(trace.read()[-4000:])
        raise
    os.dup2(saved, 2)


def run(args, trace):
    import numpy as np
    from pinot_amd import _lib as L
    from pinot_amd.executor import GpuTable
    from pinot_amd.query import FilterContext, Predicate, parse_query
    from pinot_amd.segment import ColumnData, SegmentBuffers

    vocab = ["/shop/%03d/cat-%02d/item-%03d.html" % (a, b, c) for a in range(100) for b in range(100) for c in range(100)]
    width = len(vocab[0])
    allb = np.frombuffer("".join(vocab).encode(), dtype=np.uint8).reshape(len(vocab), width)
    schema = [("g", "INT"), ("url", "STRING")]
    t = GpuTable(schema)
    rng = np.random.default_rng(5)
    hs = []
    gdict = _be32(np.arange(256))
    for i in range(args.segments):
        keep = np.flatnonzero((np.arange(len(vocab)) * 7 + i) % 4 != 0)
        ids = rng.integers(0, len(keep), args.docs)
        ids[:len(keep)] = np.arange(len(keep))[:args.docs]  # every value of the segment's dictionary occurs
        url = ColumnData(L.STRING, len(keep), 20, width, allb[keep].tobytes(), _pack20(ids))
        g = ColumnData(L.INT, 256, 8, 4, gdict, rng.integers(0, 256, args.docs).astype(np.uint8).tobytes())
        hs.append(t.pin_segment(SegmentBuffers(args.docs, {"g": g, "url": url})))
    assert len(t.dictionary("url")) == len(vocab)

    def measure(q):
        q.no_plan_cache = True
        q.timing = True
        t0 = time.perf_counter()
        p = t.plan(hs, q)
        t1 = time.perf_counter()
        p.execute()
        r = p.finalize()
        t2 = time.perf_counter()
        steady = []
        for _ in range(args.steps):
            p.execute()
            p.finalize()
            steady.append(p.timing_us()[0])
        out = {"plan_create_us": (t1 - t0) * 1e6, "first_execute_us": (t2 - t1) * 1e6,
               "steady_execute_us": statistics.median(steady), "leaf_kinds": p.leaf_kinds(), "group_path": p.group_path(),
               "docs_scanned": r.stats.as_tuple()[0], "entries_in_filter": r.stats.as_tuple()[1]}
        if hasattr(p, "regexp_stats") and not args.in_only:
            out["regexp_stats"] = p.regexp_stats()
        p.close()
        return r.as_dict(), out

    out = {"tool": "regexp_cost", "segments": args.segments, "docs_per_segment": args.docs, "steps": args.steps,
           "dictionary_values": len(vocab), "value_bytes": width, "patterns": PATTERNS, "in_only": args.in_only}
    measure(parse_query("SELECT COUNT(*) FROM t WHERE g < 3 GROUP BY g"))  # warms the context, the LUT of g, the scratch
    if not args.in_only:  # the one-off work of the first REGEXP_LIKE plan: the dictionary's upload and the segments' LUTs
        q0 = parse_query("SELECT COUNT(*) FROM t GROUP BY g")
        q0.filter = FilterContext.pred(Predicate.regexp_like("url", "zzz"))
        out["first_regexp_plan_with_upload_and_luts_us"] = measure(q0)[1]["plan_create_us"]
    for name, pattern in PATTERNS.items():
        rx = re.compile(pattern, re.IGNORECASE | re.ASCII)
        hits = [v for v in vocab if rx.search(v)]
        q_in = parse_query("SELECT COUNT(*) FROM t GROUP BY g")
        q_in.filter = FilterContext.pred(Predicate.in_("url", hits))
        got_in, m_in = measure(q_in)
        res = {"matching_values": len(hits), "in": m_in}
        if not args.in_only:
            res["dfa"] = dict(zip(("states", "classes", "table_bytes"), L.regex_check(pattern)))
            q_rx = parse_query("SELECT COUNT(*) FROM t GROUP BY g")
            q_rx.filter = FilterContext.pred(Predicate.regexp_like("url", pattern))
            pos = os.path.getsize(trace.name)
            got_rx, m_rx = measure(q_rx)
            assert got_rx == got_in and m_rx["docs_scanned"] == m_in["docs_scanned"], name
            trace.seek(pos)
            line = [x for x in trace.read().splitlines() if x.startswith("[pgpu] regex ")][-1]
            f = dict(zip(line.split()[2::2], line.split()[3::2]))  # "column url values 1000000 ... segments 20:" pairs
            k = dict(zip(line.split(": ", 1)[1].split()[0::2], line.split(": ", 1)[1].split()[1::2]))
            m_rx["match_kernel_us"] = float(k["match_us"])
            m_rx["local_sets_kernel_us"] = float(k["local_sets_us"])
            m_rx["device_round_trip_us"] = float(k["run_us"])
            m_rx["dict_device_bytes"] = int(f["dict_bytes"])
            m_rx["match_kernel_gbytes_per_s"] = int(f["dict_bytes"]) / float(k["match_us"]) / 1e3
            res["regexp_like"] = m_rx
        out[name] = res
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
