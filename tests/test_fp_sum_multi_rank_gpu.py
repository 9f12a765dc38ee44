"""Bit-reproducible FLOAT / DOUBLE sums across ranks: two ranks on one GPU agree on the fixed-point formats
(GpuTable.fp_sum_ranges -> combine.agree_fp_sum_ranges / agree_fp_sum_ranges_group -> GpuTable.plan(...,
fp_sum_ranges=...)), run agreed plans, and merge them by every combine mode -- over torch.distributed (gloo, the
collectives of pinot_amd.combine) and over the C ABI communicator's host transport (pgpu_plan_combine /
pgpu_result_combine_rows).  After the scan the digits are int64 SUM rows, so the merged answer must be the same bits
for every assignment of segments to ranks and equal to one rank holding all of them: math.fsum over the operands of
all ranks' docs per group, compared with float.hex as tests/test_fp_sum_exact_gpu.py does.

Data: rank 0's segments (8193 and 33 docs) hold only large operands, odd multiples of 4 near +-2^54 and +-2^53; rank
1's (8193 docs and 1 doc) only odd multiples of 2^-20 and 2^-30.  The ranks' own (E, L) are (55, 2) and (<= -2, -30),
the agreed ones (55, -30) -- the workers assert that before planning -- and 16 420 docs keep W = 2 exact.

Cases (every one on both transports, with the segments dealt both ways and on a single rank):
  all_reduce      GROUP BY d: 63 keys, into a caller-owned table;
  reduce_scatter  the same table sharded: 63 keys over 2 ranks, so the rows are padded;
  partitioned     GROUP BY a1, a2: 10^6 keys x 6 slots, radix-partitioned (K8d FX) on both ranks, reduce-scattered;
  hash            GROUP BY h1, h2: hashed partitions (K8h FX), materialised as a table, exchanged on the device;
  rows            GROUP BY d, f under a numGroupsLimit that makes the plan composite: finalized rows exchanged;
  star            one star-tree segment per rank, all-reduced (operands: the pre-aggregated doubles).
The workers run everything once per transport and dump what they got; the tests only compare.
"""
import ast
import datetime
import json
import math
import os
import socket
import time

import numpy as np
import pytest

import startree_common as SC
from pinot_amd import _lib as L
from pinot_amd.query import parse_query

pytestmark = pytest.mark.gpu

WORLD = 2
SCHEMA = [("d", "INT"), ("h1", "INT"), ("h2", "INT"), ("a1", "INT"), ("a2", "INT"), ("f", "INT"), ("x", "DOUBLE")]
CARDS = {"d": 63, "h1": 9000, "h2": 9000, "a1": 1000, "a2": 1000, "f": 1000}
# segment -> (docs, kind); SETS[s]: the segments of one rank
SEGMENTS = [(8193, "large54"), (33, "large53"), (8193, "small20"), (1, "small30")]
SETS = [(0, 1), (2, 3)]
LIMIT = 20000
DENSE6 = "SELECT SUM(x), COUNT(*), MIN(f), MAX(f), SUM(f) FROM t GROUP BY a1, a2"
# name -> (sql, numGroupsLimit, group-by columns, shard, combine mode, group path on every rank)
CASES = {
    "all_reduce": ("SELECT SUM(x), COUNT(*) FROM t GROUP BY d", 10 ** 9, ("d",), False, "dense", "lds"),
    "reduce_scatter": ("SELECT SUM(x), COUNT(*) FROM t GROUP BY d", 10 ** 9, ("d",), True, "dense", "lds"),
    "partitioned": (DENSE6, 10 ** 9, ("a1", "a2"), True, "dense", "partitioned"),
    "hash": ("SELECT SUM(x), COUNT(*) FROM t GROUP BY h1, h2", 10 ** 9, ("h1", "h2"), False, "hash", "hash_partitioned"),
    "rows": ("SELECT SUM(x), COUNT(*) FROM t GROUP BY d, f", LIMIT, ("d", "f"), False, "rows", None),
}
STAR_SQL = "SELECT SUM(md), COUNT(*) FROM t GROUP BY d3"
STAR_DOCS = 3000


def segment_columns(s):
    n, kind = SEGMENTS[s]
    rng = np.random.default_rng(700 + s)
    cols = {c: rng.integers(0, card, n).astype(np.int64) for c, card in CARDS.items()}
    for c in ("h1", "h2"):
        cols[c] = rng.integers(0, 30, n).astype(np.int64) * 250 + 7
    if kind.startswith("large"):
        base = 2.0 ** int(kind[5:])
        big = base + 4.0 * (2 * rng.integers(0, 500, n) + 1)
        cols["x"] = np.where(rng.integers(0, 2, n) == 0, big, -big)
    else:
        cols["x"] = (2 * rng.integers(0, 100000, n) + 1) * 2.0 ** -int(kind[5:])
    return cols


def star_columns(s):
    """Star-tree segment s: rank 0's pre-aggregates come from large operands, rank 1's from small ones."""
    rng = np.random.default_rng(900 + s)
    cols = SC.c4_columns(rng, STAR_DOCS, cards=(40, 15, 8, 6))
    if s == 0:
        big = 2.0 ** 54 + 4.0 * (2 * rng.integers(0, 500, STAR_DOCS) + 1)
        cols["md"] = np.where(rng.integers(0, 2, STAR_DOCS) == 0, big, -big)
    else:
        cols["md"] = (2 * rng.integers(0, 100000, STAR_DOCS) + 1) * 2.0 ** -30
    return cols


def _star_tree(seg):
    from pinot_amd.startree import StarTree
    return StarTree.build(SC.C4_SCHEMA, seg, SC.C4_SPLIT, SC.C4_PAIRS, max_leaf_records=300)


def _dump(path, res, **extra):
    out = {repr(tuple(k)): [float(v[0]).hex()] + [float(x) for x in v[1:]] for k, v in res.as_dict().items()}
    with open(path, "w") as f:
        json.dump({"groups": out, **extra}, f)


# ------------------------------------------------------------------------------------------------- the workers
class _Torch:
    def __init__(self, rank, port, uid):
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        # a rank that dies must not leave the other waiting in a collective
        dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=60))

    def union(self, table, cols):
        from pinot_amd.combine import union_dictionaries
        union_dictionaries(table, cols)

    def agree(self, ranges):
        from pinot_amd.combine import agree_fp_sum_ranges_group
        return agree_fp_sum_ranges_group(ranges)

    def query(self, table, hs, q, stream, ranges, shard):
        import torch
        from pinot_amd.combine import (allreduce_group_table, exchange_hash_table, exchange_result, plan_combine_mode,
                                       reduce_scatter_group_table)
        mode = plan_combine_mode(table, hs, q, fp_sum_ranges=ranges)
        if mode == "dense":
            with table.plan(hs, q, fp_sum_ranges=ranges) as probe:
                nslots, nkeys, kinds = probe.layout()
            d_table = torch.empty((nslots, nkeys), dtype=torch.int64, device="cuda")
            plan = table.plan_execute(hs, q, stream, d_table.data_ptr(), fp_sum_ranges=ranges)
            if shard:
                part, k0, kn = reduce_scatter_group_table(d_table, kinds)
                res = plan.finalize_range(stream, part.data_ptr(), k0, kn)
            else:
                allreduce_group_table(d_table, kinds)
                res = plan.finalize(stream, d_table.data_ptr())
        elif mode == "hash":
            plan = table.plan_execute(hs, q, stream, fp_sum_ranges=ranges)
            exchange_hash_table(plan)
            res = plan.finalize(stream)
        else:
            plan = table.plan_execute(hs, q, stream, fp_sum_ranges=ranges)
            res = exchange_result(table, plan.finalize(stream))
        return mode, plan, res

    def negatives(self, table, hs, q, stream):
        return {}

    def close(self):
        import torch.distributed as dist
        dist.destroy_process_group()


class _Comm:
    def __init__(self, rank, port, uid):
        from pinot_amd.combine import Communicator
        self.comm = Communicator(L.COMM_HOST, uid, WORLD, rank, 0)
        self.comm.set_timeout(60000)

    def union(self, table, cols):
        from pinot_amd.combine import union_dictionaries_comm
        union_dictionaries_comm(table, cols, self.comm)

    def agree(self, ranges):
        from pinot_amd.combine import agree_fp_sum_ranges
        return agree_fp_sum_ranges(ranges, self.comm)

    def query(self, table, hs, q, stream, ranges, shard):
        import torch
        from pinot_amd.combine import combine_mode, combine_plan, combine_result_rows
        with table.plan(hs, q, fp_sum_ranges=ranges) as probe:
            mode, kinds = combine_mode(probe, self.comm, 0 if shard else 1 << 62)
            nslots, nkeys = (probe.layout()[:2] if mode in (L.COMBINE_ALL_REDUCE, L.COMBINE_REDUCE_SCATTER) else (0, 0))
        if mode in (L.COMBINE_ALL_REDUCE, L.COMBINE_REDUCE_SCATTER):
            assert mode == (L.COMBINE_REDUCE_SCATTER if shard else L.COMBINE_ALL_REDUCE), mode
            d_table = None if shard else torch.empty((nslots, nkeys), dtype=torch.int64, device="cuda")
            ptr = d_table.data_ptr() if d_table is not None else None
            plan = table.plan_execute(hs, q, stream, ptr, fp_sum_ranges=ranges)
            combine_plan(plan, self.comm, stream, mode, kinds, d_table=ptr)
            return "dense", plan, plan.finalize(stream, ptr)
        plan = table.plan_execute(hs, q, stream, fp_sum_ranges=ranges)
        if mode == L.COMBINE_HASH:
            combine_plan(plan, self.comm, stream, mode, kinds)
            return "hash", plan, plan.finalize(stream)
        assert mode == L.COMBINE_ROWS, mode
        return "rows", plan, combine_result_rows(table, plan.finalize(stream), self.comm)

    def negatives(self, table, hs, q, stream):
        """Every rank plans with its *own* ranges: the formats differ, and the mode agreement says so on every rank
        (a collective: both ranks call it).  A plain plan is declined before any exchange."""
        from pinot_amd.combine import combine_mode
        out = {}
        with table.plan(hs, q, fp_sum_ranges=table.fp_sum_ranges(hs, q)) as own:
            try:
                combine_mode(own, self.comm, 1 << 62)
                out["own_ranges"] = "no error"
            except L.PinotGpuError as e:
                out["own_ranges"] = [e.code, e.message]
        with table.plan(hs, q) as plain:
            try:
                combine_mode(plain, self.comm, 1 << 62)
                out["plain"] = "no error"
            except L.UnsupportedQueryError as e:
                out["plain"] = [e.code, e.message]
        return out

    def close(self):
        self.comm.close()


def _table(segs):
    import _oracle
    from pinot_amd.executor import GpuTable
    t = GpuTable(SCHEMA, device=0)
    for c, card in CARDS.items():  # one key space on every rank
        t.add_dictionary_values(c, list(range(card)))
    return t, [t.pin_segment(_oracle.make_segment(SCHEMA, segment_columns(s))) for s in segs]


def _star_table(segs):
    import _oracle
    from pinot_amd.executor import GpuTable
    t = GpuTable(SC.C4_SCHEMA, device=0)
    hs = []
    for s in segs:
        seg = _oracle.make_segment(SC.C4_SCHEMA, star_columns(s))
        hs.append(t.pin_segment(seg))
        t.attach_startree(hs[-1], _star_tree(seg))
    return t, hs


def _worker(rank, port, out_dir, transport, uid):
    import torch
    merge = (_Torch if transport == "torch" else _Comm)(rank, port, uid)
    try:
        torch.cuda.set_device(0)
        torch.cuda.set_stream(torch.cuda.Stream())  # (handle 0 would mean "the table's own stream" to the C ABI)
        stream = torch.cuda.current_stream().cuda_stream
        for deal in (0, 1):
            table, hs = _table(SETS[rank ^ deal])
            for name, (sql, limit, _, shard, _, _) in CASES.items():
                q = parse_query(sql, num_groups_limit=limit, exact_fp_sum=True)
                mine = table.fp_sum_ranges(hs, q)
                agreed = merge.agree(mine)
                # the ranks' own ranges differ from each other and from the agreed one
                large = (rank ^ deal) == 0
                assert (mine[0].E, mine[0].L) == ((55, 2) if large else (mine[0].E, -30)) and (large or mine[0].E <= -2)
                assert (agreed[0].E, agreed[0].L, agreed[0].docs) == (55, -30, sum(n for n, _ in SEGMENTS)), agreed[0].as_tuple()
                mode, plan, res = merge.query(table, hs, q, stream, agreed, shard)
                _dump(os.path.join(out_dir, "%s_%d_%d.json" % (name, deal, rank)), res, mode=mode,
                      group_path=plan.group_path(), fmt=plan.fp_sum_format(0))
                plan.close()
            if deal == 0:
                q = parse_query(CASES["all_reduce"][0], exact_fp_sum=True)
                with open(os.path.join(out_dir, "negatives_%d.json" % rank), "w") as f:
                    json.dump(merge.negatives(table, hs, q, stream), f)
            table.close()
            # star-tree: one segment per rank, the group-by dictionaries unioned, all-reduced
            t4, h4 = _star_table([rank ^ deal])
            merge.union(t4, ["d3"])
            q4 = parse_query(STAR_SQL, num_groups_limit=10 ** 9, exact_fp_sum=True)
            agreed = merge.agree(t4.fp_sum_ranges(h4, q4))
            mode, plan, res = merge.query(t4, h4, q4, stream, agreed, False)
            _dump(os.path.join(out_dir, "star_%d_%d.json" % (deal, rank)), res, mode=mode, group_path=plan.group_path(),
                  fmt=plan.fp_sum_format(0), star_segments=plan.star_work()[0])
            plan.close()
            t4.close()
        if rank == 0:  # one rank holding every segment: agreed = its own ranges, nothing to merge
            table, hs = _table(range(len(SEGMENTS)))
            for name, (sql, limit, _, _, _, _) in CASES.items():
                q = parse_query(sql, num_groups_limit=limit, exact_fp_sum=True)
                with table.plan_execute(hs, q, stream, fp_sum_ranges=table.fp_sum_ranges(hs, q)) as plan:
                    _dump(os.path.join(out_dir, "%s_single.json" % name), plan.finalize(stream), group_path=plan.group_path(),
                          fmt=plan.fp_sum_format(0))
            table.close()
            t4, h4 = _star_table([0, 1])
            q4 = parse_query(STAR_SQL, num_groups_limit=10 ** 9, exact_fp_sum=True)
            with t4.plan_execute(h4, q4, stream, fp_sum_ranges=t4.fp_sum_ranges(h4, q4)) as plan:
                _dump(os.path.join(out_dir, "star_single.json"), plan.finalize(stream), fmt=plan.fp_sum_format(0))
            t4.close()
    finally:
        merge.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(out_dir, transport, limit_s=240):
    import torch.multiprocessing as mp
    from pinot_amd.combine import Communicator
    uid = Communicator.unique_id(L.COMM_HOST) if transport == "comm" else None
    ctx = mp.spawn(_worker, args=(_free_port(), str(out_dir), transport, uid), nprocs=WORLD, join=False)
    t0 = time.time()
    while not ctx.join(timeout=2):  # (raises when a rank died: the run ends instead of hanging)
        if time.time() - t0 > limit_s:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail("ranks did not finish within %d s" % limit_s)


@pytest.fixture(scope="module")
def runs(gpu_lib, tmp_path_factory):
    """transport -> the directory its two ranks dumped into; each transport is spawned once, on first use."""
    done = {}

    def get(transport):
        if transport not in done:
            done[transport] = tmp_path_factory.mktemp("fp_sum_ranks_" + transport)
            _run_ranks(done[transport], transport)
        return done[transport]
    return get


# ---------------------------------------------------------------------------------------------- the references
def _groups(keys, cols_of_segments, col):
    out = {}
    for cols in cols_of_segments:
        for i in range(len(cols[col])):
            out.setdefault(tuple(int(cols[k][i]) for k in keys), []).append(float(cols[col][i]))
    return out


@pytest.fixture(scope="module")
def reference():
    """name -> {key: (hex of math.fsum over the operands of all ranks' docs, count)}; computed once."""
    segs = [segment_columns(s) for s in range(len(SEGMENTS))]
    cache = {}

    def get(name):
        keys = CASES[name][2]
        if keys not in cache:
            cache[keys] = {k: (math.fsum(v).hex(), len(v)) for k, v in _groups(keys, segs, "x").items()}
        return cache[keys]
    return get


@pytest.fixture(scope="module")
def star_reference(oracle):
    """The star path's operands are the pre-aggregated doubles of the star-tree documents the traversal selects."""
    from test_fp_sum_exact_gpu import _star_selected
    q = parse_query(STAR_SQL)
    groups = {}
    for s in range(WORLD):
        seg = oracle.make_segment(SC.C4_SCHEMA, star_columns(s))
        (ids,), vals = _star_selected(_star_tree(seg).arrays(), seg, q)
        d3 = SC.dictionary_values(seg.columns["d3"])
        for g in np.unique(ids):
            groups.setdefault((int(d3[g]),), []).extend(vals[ids == g].tolist())
    return {k: math.fsum(v).hex() for k, v in groups.items()}


def _load(path):
    with open(path) as f:
        z = json.load(f)
    z["groups"] = {ast.literal_eval(k): v for k, v in z["groups"].items()}  # (reprs of int tuples)
    return z


def _merged(parts, everywhere):
    """The ranks' shares as one answer: equal on every rank after an all-reduce, else disjoint."""
    a, b = parts[0]["groups"], parts[1]["groups"]
    if everywhere:
        assert a == b
        return a
    assert not set(a) & set(b)
    return {**a, **b}


# ------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("transport", ["torch", "comm"])
def test_merged_sums_are_bit_equal_to_fsum_however_the_segments_are_dealt(runs, reference, transport, name):
    out = runs(transport)
    _, _, _, shard, mode, path = CASES[name]
    want = reference(name)
    merged = []
    for deal in (0, 1):
        parts = [_load(out / ("%s_%d_%d.json" % (name, deal, r))) for r in range(WORLD)]
        for p in parts:
            assert p["mode"] == mode, p["mode"]
            assert path is None or p["group_path"] == path, "rank ran on the %s path" % p["group_path"]
            assert p["fmt"]["mode"] == "exact" and p["fmt"]["W"] == 2 and p["fmt"]["E"] == 55, p["fmt"]
            assert p["fmt"] == parts[0]["fmt"]
        merged.append(_merged(parts, everywhere=name == "all_reduce"))
    got = merged[0]
    assert set(got) == set(want)
    bad = [(k, got[k][0], want[k][0]) for k in want if got[k][0] != want[k][0]]
    assert not bad, "%d of %d groups differ from math.fsum, e.g. %s" % (len(bad), len(want), bad[:3])
    assert all(got[k][1] == want[k][1] for k in want)  # COUNT(*)
    assert merged[1] == got, "the answer depends on which rank holds which segments"
    single = _load(out / ("%s_single.json" % name))
    assert single["groups"] == got, "two ranks and one rank give different answers"
    assert single["fmt"] == _load(out / ("%s_0_0.json" % name))["fmt"]


@pytest.mark.parametrize("transport", ["torch", "comm"])
def test_star_tree_plans_merge_bit_equal_to_fsum(runs, star_reference, transport):
    out = runs(transport)
    merged = []
    for deal in (0, 1):
        parts = [_load(out / ("star_%d_%d.json" % (deal, r))) for r in range(WORLD)]
        for p in parts:
            assert p["mode"] == "dense" and p["star_segments"] == 1, p
            assert p["fmt"]["mode"] == "exact" and p["fmt"] == parts[0]["fmt"], p["fmt"]
        merged.append(_merged(parts, everywhere=True))
    got = {k: v[0] for k, v in merged[0].items()}
    assert got == star_reference
    assert merged[1] == merged[0]
    assert _load(out / "star_single.json")["groups"] == merged[0]


def test_ranks_with_their_own_ranges_are_refused_and_plain_plans_declined(runs):
    out = runs("comm")
    for r in range(WORLD):
        with open(out / ("negatives_%d.json" % r)) as f:
            neg = json.load(f)
        assert neg["own_ranges"][0] == L.PGPU_ERR_INVALID_ARGUMENT and "fixed-point formats" in neg["own_ranges"][1], neg
        assert neg["plain"][0] == L.PGPU_ERR_UNSUPPORTED and "PGPU_OPT_EXACT_FP_SUM" in neg["plain"][1], neg


def test_one_rank_rccl_communicator_combines_agreed_plans(oracle, gpu_lib, reference):
    """The real RCCL calls see the digit rows: ALL_REDUCE and REDUCE_SCATTER of an agreed plan on a one-rank
    communicator give the single-rank answer; the plain plan is still declined."""
    from pinot_amd.combine import Communicator, combine_mode, combine_plan
    table, hs = _table(range(len(SEGMENTS)))
    comm = Communicator(L.COMM_RCCL, Communicator.unique_id(L.COMM_RCCL), 1, 0, 0)
    try:
        q = parse_query(CASES["all_reduce"][0], exact_fp_sum=True)
        ranges = table.fp_sum_ranges(hs, q)
        want = reference("all_reduce")
        for shard_bytes, want_mode in ((1 << 62, L.COMBINE_ALL_REDUCE), (0, L.COMBINE_REDUCE_SCATTER)):
            with table.plan_execute(hs, q, fp_sum_ranges=ranges) as p:
                mode, kinds = combine_mode(p, comm, shard_bytes)
                assert mode == want_mode
                assert kinds == [L.SLOT_COUNT, L.SLOT_SUM_I64, L.SLOT_SUM_I64]  # the digits travel as int64 sums
                combine_plan(p, comm, None, mode, kinds)
                got = p.finalize().as_dict()
            assert {k: (float(v[0]).hex(), v[1]) for k, v in got.items()} == want
        with table.plan_execute(hs, q) as p:
            with pytest.raises(L.UnsupportedQueryError, match="PGPU_OPT_EXACT_FP_SUM"):
                combine_mode(p, comm, 1 << 62)
    finally:
        comm.close()
        table.close()
