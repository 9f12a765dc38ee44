"""Result signature of one fixed list of small queries, one JSON line per query: group path, table layout, groups,
the six statistics, numGroupsLimitReached, star-tree docs read / metric bytes, the finalize branch named by the
library's `[pgpu] finalize:` trace line (libraries that print it) and a SHA-1 of the decoded rows.  The list reaches
every finalize branch (rt_finalize.cpp) once.  Two libraries compute the same when their files are equal:

  PGPU_TRACE=1 PGPU_LIB=<a.so> python tools/result_signature.py --out a.jsonl
  PGPU_TRACE=1 python tools/result_signature.py --out b.jsonl
  python tools/result_signature.py --compare a.jsonl b.jsonl     # fields absent from the first file are ignored

Run the first library twice and compare its two files first: a query whose signature differs between them does not
belong in the list.

FLOAT / DOUBLE sums under the default atomics depend on the order of the adds: the list sums integer columns, or
asks for exact_fp_sum."""
import argparse
import ctypes
import hashlib
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from pinot_amd import _lib as L  # noqa: E402


class _Stderr:
    """The process's stderr (the library's trace lines) captured into .text."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        sys.stderr.write(self.text)


def _canon(v):
    if isinstance(v, float):
        return float(v).hex()
    if hasattr(v, "sum") and hasattr(v, "count"):  # AvgPair
        return [_canon(v.sum), int(v.count)]
    if isinstance(v, (list, tuple)):
        return [_canon(x) for x in v]
    if isinstance(v, (np.floating,)):
        return float(v).hex()
    if isinstance(v, (np.integer, int)):
        return int(v)
    return str(v)


def signature(name, plan, finalize):
    """finalize: callable returning the GroupByResult of the executed plan."""
    with _Stderr() as err:
        res = finalize()
    rows = sorted((repr(k), _canon(v)) for k, v in res.as_dict().items())
    st = res.stats
    m = re.findall(r"\[pgpu\] finalize:.*?\(n=(-?\d+)\)(?: branch (\S+))?", err.text)

    def ask(fn):  # (a numGroupsLimit plan split into parts has no table of its own: null)
        try:
            return fn()
        except L.UnsupportedQueryError:
            return None
    sig = {"name": name, "group_path": ask(plan.group_path), "layout": ask(lambda: list(plan.layout())),
           "groups": len(res),
           "stats": [st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_entries_scanned_post_filter,
                     st.num_total_docs, st.num_segments_processed, st.num_segments_matched], "limit_reached": bool(res.num_groups_limit_reached),
           "star_docs_read": ask(lambda: int(plan.star_work()[2])),
           "star_metric_bytes": ask(lambda: int(plan.star_metric_bytes())),
           "rows_sha1": hashlib.sha1(json.dumps(rows).encode()).hexdigest()}
    if m and m[-1][1]:
        sig["finalize_branch"] = m[-1][1]
    return sig


def run(out_path):
    import torch
    import _oracle as oracle
    import kat_common as K
    import startree_common as SC
    from pinot_amd.executor import GpuTable
    from pinot_amd.query import parse_query
    from pinot_amd.startree import StarTree

    oracle.lib()
    torch.cuda.set_stream(torch.cuda.Stream())  # a real stream (handle 0 is the table's own to the C ABI)
    stream = torch.cuda.current_stream().cuda_stream
    sigs = []

    def plain(name, t, hs, sql, **opts):
        q = parse_query(sql, **opts) if isinstance(sql, str) else sql
        p = t.plan_execute(hs, q)
        try:
            sigs.append(signature(name, p, p.finalize))
        finally:
            p.close()

    # -- sparse key spaces: LDS table, K8h's records, the global hash table (tests/test_hash_partition_gpu.py's shape)
    schema = [("a", "INT"), ("b", "INT"), ("c", "INT"), ("m", "INT"), ("x", "DOUBLE"), ("s", "INT")]
    docs = 120000

    def cols(seed):
        rng = np.random.default_rng(seed)
        return {"a": rng.integers(0, 3000, docs).astype(np.int64), "b": rng.integers(0, 3000, docs).astype(np.int64),
                "c": rng.integers(0, 30, docs).astype(np.int64), "m": rng.integers(-400, 900, docs).astype(np.int64),
                "x": np.round(rng.uniform(-1e4, 1e4, docs), 3), "s": rng.integers(0, 100, docs).astype(np.int64)}
    t = GpuTable(schema)
    hs = [t.pin_segment(oracle.make_segment(schema, cols(41 + s))) for s in range(2)]
    big = 10 ** 9
    try:
        plain("small_dense/internal", t, hs, "SELECT COUNT(*), SUM(m), MIN(x) FROM t GROUP BY c", num_groups_limit=big)
        q = parse_query("SELECT COUNT(*), SUM(m) FROM t WHERE m > 0 GROUP BY c, s", num_groups_limit=big)
        with t.plan(hs, q) as p:  # the caller's table: statistics apart from it
            ns, nk, _ = p.layout()
            d = torch.empty((ns, nk), dtype=torch.int64, device="cuda")
            p.execute(stream, d.data_ptr())
            sigs.append(signature("small_dense/caller_table", p, lambda: p.finalize(stream, d.data_ptr())))
        plain("small_dense/generic_filter", t, hs, "SELECT COUNT(*), SUM(m) FROM t WHERE (a < 900 OR b > 2000) AND "
              "NOT (c = 2 OR (m < 100 AND s > 50)) GROUP BY c", num_groups_limit=big)
        plain("small_dense/exact_fp_sum", t, hs, "SELECT SUM(x), AVG(x), COUNT(*) FROM t WHERE m > 0 GROUP BY c",
              num_groups_limit=big, exact_fp_sum=True)
        k8h = "SELECT COUNT(*), SUM(m), MAX(x) FROM t%s GROUP BY a, b, c"
        glob = "SELECT COUNT(*), SUM(m), MAX(x) FROM t%s GROUP BY a, b, c, s"
        for tag, sql in (("k8h", k8h), ("hash_global", glob)):
            plain(tag + "/compact", t, hs, sql % "", num_groups_limit=big)
            plain(tag + "/sorted", t, hs, sql % " WHERE m = 5 AND s < 30", num_groups_limit=big)  # < 4096 groups
            # (exact_fp_sum over either key list runs the global hash table, not K8h)
            plain("hash_global/exact_fp_sum_%dkeys" % (3 if tag == "k8h" else 4), t, hs, "SELECT SUM(x), COUNT(*) FROM t "
                  "GROUP BY a, b, c" + (", s" if tag == "hash_global" else ""), num_groups_limit=big, exact_fp_sum=True)
            plain(tag + "/pql_groups_limit", t, hs, sql % "", num_groups_limit=5000)
            t.set_config(compact_results=0)
            try:
                plain(tag + "/decoded", t, hs, sql % "", num_groups_limit=big)
            finally:
                t.reset_config()
        q = parse_query("SELECT COUNT(*), SUM(m) FROM t GROUP BY a, b, c", num_groups_limit=big)
        p = t.plan_execute(hs, q)  # a hash table after exchange + merge (one rank): merged_records >= 0
        try:
            counts = p.exchange_counts(None, 1)
            rec = torch.empty((int(counts[0]), 3), dtype=torch.int64, device="cuda")
            d_rec, n_rec = ctypes.c_void_p(rec.data_ptr()), int(counts[0])
            L.check(p.lib.pgpu_plan_exchange_export(p.handle, None, 1, None, d_rec, n_rec))
            L.check(p.lib.pgpu_plan_exchange_merge(p.handle, None, None, d_rec, n_rec))
            sigs.append(signature("hash_merged/after_exchange", p, p.finalize))
        finally:
            p.close()
    finally:
        t.close()

    # -- large dense tables (tests/test_gpu_parity.py's C5 shape): compact, columnar, K8d's counts, no group
    rng = np.random.default_rng(150000)
    dschema = [("k1", "INT"), ("k2", "INT"), ("k3", "INT"), ("m", "INT"), ("q", "INT")]
    dsegs = [oracle.make_segment(dschema, {"k1": rng.integers(0, 400, 150000), "k2": rng.integers(0, 60, 150000),
                                           "k3": rng.integers(0, 50, 150000), "m": rng.integers(0, 1000, 150000),
                                           "q": rng.integers(-500, 500, 150000)}) for _ in range(2)]
    for tag, cfg in (("partitioned", None), ("atomics", {"partitioned_group_by": 0})):
        t = GpuTable(dschema, config=cfg)
        hs = [t.pin_segment(s) for s in dsegs]
        try:
            plain("large_dense/%s/count_sum" % tag, t, hs, "SELECT SUM(m), COUNT(*) FROM t GROUP BY k1, k2, k3",
                  num_groups_limit=10 ** 7)
            plain("large_dense/%s/compact" % tag, t, hs, "SELECT SUM(q), MIN(q), MAX(m), COUNT(*) FROM t WHERE q < 0 "
                  "OR m > 900 GROUP BY k1, k2, k3", num_groups_limit=10 ** 7)
            plain("large_dense/%s/no_group" % tag, t, hs, "SELECT SUM(m), COUNT(*) FROM t WHERE q > 400 AND q < -400 "
                  "GROUP BY k1, k2, k3", num_groups_limit=10 ** 7)
            t.set_config(compact_results=0)
            plain("large_dense/%s/columnar" % tag, t, hs, "SELECT SUM(m), COUNT(*), MIN(q) FROM t GROUP BY k1, k2, k3",
                  num_groups_limit=10 ** 7)
        finally:
            t.close()

    # -- K8d's chunk counts: COUNT + SUM over a table past the partitioned pipeline's threshold
    rng = np.random.default_rng(8)
    kschema = [("k1", "INT"), ("k2", "INT"), ("k3", "INT"), ("m", "INT")]
    kseg = oracle.make_segment(kschema, {"k1": rng.integers(0, 400, 150000), "k2": rng.integers(0, 60, 150000),
                                         "k3": rng.integers(0, 200, 150000), "m": rng.integers(0, 1000, 150000)})
    t = GpuTable(kschema)
    try:
        plain("large_dense/k8d_counts", t, [t.pin_segment(kseg)], "SELECT SUM(m), COUNT(*) FROM t GROUP BY k1, k2, k3",
              num_groups_limit=10 ** 7)
    finally:
        t.close()

    # -- key-range shards of a caller's dense table (finalize_range, key_begin > 0)
    from pinot_amd.combine import shard_range
    rng = np.random.default_rng(7)
    rschema = [("a", "INT"), ("b", "INT"), ("m", "INT")]
    seg = oracle.make_segment(rschema, {"a": rng.integers(0, 300, 120000), "b": rng.integers(0, 200, 120000),
                                        "m": rng.integers(0, 1000, 120000)})
    t = GpuTable(rschema)
    hs = [t.pin_segment(seg)]
    try:
        q = parse_query("SELECT COUNT(*), SUM(m) FROM t WHERE m < 900 GROUP BY a, b", num_groups_limit=10 ** 6)
        with t.plan(hs, q) as p:
            ns, nk, _ = p.layout()
            d = torch.empty((ns, nk), dtype=torch.int64, device="cuda")
            p.execute(stream, d.data_ptr())
            sigs.append(signature("large_dense/caller_table", p, lambda: p.finalize(stream, d.data_ptr())))
            for r in (1, 2):
                k0, kn, _ = shard_range(nk, 3, r)
                shard = d[:, k0:k0 + kn].contiguous()
                sigs.append(signature("small_dense/range_shard_%d" % r, p,
                                      lambda: p.finalize_range(stream, shard.data_ptr(), k0, kn)))
    finally:
        t.close()

    # -- ARRAY_MAP stages (the reference KAT's 9 group-by columns)
    t = GpuTable(K.SCHEMA)
    hs = [t.pin_segment(K.kat_segment(oracle, pairs=True))]
    try:
        case = K.KAT["inner_segment_group_by"][3]
        for name, flt, limit in (("array_map/all", False, big), ("array_map/filter", True, big),
                                 ("array_map/groups_limit", False, 1000)):
            q = K.inner_query(case["group_by"], flt)
            q.num_groups_limit = limit
            plain(name, t, hs, q)
    finally:
        t.close()

    # -- star-tree segments (tests/test_startree_gpu.py's shape): the statistics' star words
    rng = np.random.default_rng(404)
    t = GpuTable(SC.C4_SCHEMA)
    try:
        hs = []
        for i in range(3):
            seg = oracle.make_segment(SC.C4_SCHEMA, SC.c4_columns(rng, 40000 + 7919 * i, cards=(40, 15, 8, 6)))
            hs.append(t.pin_segment(seg))
            t.attach_startree(hs[-1], StarTree.build(SC.C4_SCHEMA, seg, SC.C4_SPLIT, SC.C4_PAIRS,
                                                     max_leaf_records=300))
        for i, sql in enumerate(SC.C4_QUERIES):
            if "SUM(md)" not in sql:  # (a DOUBLE sum under atomics)
                plain("star_tree/%d" % i, t, hs, sql, num_groups_limit=big)
    finally:
        t.close()

    with open(out_path, "w") as f:
        for s in sigs:
            f.write(json.dumps(s, sort_keys=True) + "\n")
    print("%d signatures -> %s" % (len(sigs), out_path))


def compare(a_path, b_path):
    def load(p):
        with open(p) as f:
            return [json.loads(line) for line in f if line.strip()]
    a, b = load(a_path), load(b_path)
    bad = len(a) != len(b)
    for x, y in zip(a, b):
        for k, v in x.items():
            if y.get(k) != v:
                bad = True
                print("%s: %s differs: %r vs %r" % (x["name"], k, v, y.get(k)))
    print("differ" if bad else "equal: %d queries" % len(a))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.out) or 0)
