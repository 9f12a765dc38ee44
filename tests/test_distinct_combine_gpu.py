"""DISTINCTCOUNT merged across GPUs in the dense combine modes of the C ABI (pgpu_plan_combine_mode / pgpu_plan_combine
on the plan's own table): the ranks' side bitmaps are reduce-scattered by key range (one all-to-all per distinct
column), ORed and popcounted by the owner (distinct_merge_popcount_kernel), and the int64 SUM of the table's own
collectives carries the counts.

Two spawned ranks share the one GPU over the host transport (the pattern of test_multi_rank_gpu.py's "comm"
transport; three processes in all).  Each rank pins 3 segments of 20 000 docs, unions the dictionaries of the group-by
and the distinct columns, runs every case once and dumps its results; the parent compares.  The worker run is shared
by the tests of this module.  The reference for DISTINCTCOUNT is distinct_common.distinct_counts over the docs of both
ranks, for COUNT / SUM / MIN / MAX brute-force numpy over the same docs; everything is compared exactly, as integers.

The distinct columns' values on the two ranks overlap partly (rank-dependent offsets), so a merge that added the
ranks' counts, or returned one rank's, cannot pass (test_data_tells_a_merge_from_a_sum_or_one_rank asserts that on
the CPU).  Cardinalities after the union: 1 (a single bit), 64 (the last bit of a full word), 65 (a last word of one
bit), 3 000 (47 words: some lanes idle), 70 000 (1 094 words: lanes stride more than once), and a STRING column."""
import os
import pickle
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import distinct_common as D
from pinot_amd import _lib as L
from pinot_amd.query import parse_query

pytestmark = pytest.mark.gpu

SCHEMA = [("d", "INT"), ("f", "INT"), ("one", "INT"), ("mi", "INT"), ("v1", "INT"), ("v64", "INT"), ("v65", "INT"),
          ("v3k", "INT"), ("v70k", "INT"), ("w", "INT"), ("s", "STRING")]
WORLD = 2
SEGS_PER_RANK = 3
DOCS = 20000
UNIONED = ["d", "f", "one", "v1", "v64", "v65", "v3k", "v70k", "s"]  # every group-by and distinct column but w
CARDS = {"d": 41, "one": 1, "v1": 1, "v64": 64, "v65": 65, "v3k": 3000, "v70k": 70000, "s": 300}
# name -> (sql, reduce-scatter?)
CASES = {
    # two distinct columns, the first counted twice (one bitmap shared by two aggregations), a filter
    "all_reduce": ("SELECT COUNT(*), DISTINCTCOUNT(v3k), SUM(mi), DISTINCTCOUNT(v70k), MIN(mi), MAX(mi), "
                   "DISTINCTCOUNT(v3k) FROM t WHERE f < 40 GROUP BY d", False),
    "word_edges": ("SELECT DISTINCTCOUNT(v1), DISTINCTCOUNT(v64), DISTINCTCOUNT(v65), DISTINCTCOUNT(s), COUNT(*) "
                   "FROM t GROUP BY d", False),
    # 41 x 27 = 1107 keys: not a multiple of the ranks (the padded reduce-scatter of the rows)
    "odd": ("SELECT COUNT(*), DISTINCTCOUNT(v65), SUM(mi), DISTINCTCOUNT(v70k), MAX(mi), DISTINCTCOUNT(s) FROM t "
            "WHERE f BETWEEN 10 AND 50 AND d BETWEEN 3 AND 29 GROUP BY f, d", True),
    # one key: the second rank owns none
    "g1_all_reduce": ("SELECT DISTINCTCOUNT(v3k), COUNT(*), DISTINCTCOUNT(v64) FROM t WHERE f < 40 GROUP BY one", False),
    "g1_reduce_scatter": ("SELECT DISTINCTCOUNT(v3k), COUNT(*), DISTINCTCOUNT(v64) FROM t WHERE f < 40 GROUP BY one", True),
}
AGAIN = ("all_reduce", "odd")  # run a second time: a plan-cache hit, combined again
MISMATCH = "SELECT DISTINCTCOUNT(w), COUNT(*) FROM t GROUP BY d"  # w was left out of the union
LIMIT = 10 ** 9


def _rank_columns(rank):
    """The 60 000 docs of one rank.  full(lo, hi): every value of [lo, hi) occurs, so the cardinalities after the
    union are exact; the ranges of the two ranks overlap partly."""
    rng = np.random.default_rng(900 + rank)
    n = SEGS_PER_RANK * DOCS

    def full(lo, hi):
        v = rng.integers(lo, hi, n)
        v[:hi - lo] = np.arange(lo, hi)
        rng.shuffle(v)
        return v.astype(np.int64)

    return {"d": full(7 * rank, 34 + 7 * rank), "f": rng.integers(0, 100, n).astype(np.int64),
            "one": np.zeros(n, dtype=np.int64), "mi": rng.integers(-5000, 70000, n).astype(np.int64),
            "v1": np.full(n, 5, dtype=np.int64), "v64": full(24 * rank, 40 + 24 * rank),
            "v65": full(25 * rank, 40 + 25 * rank), "v3k": full(1000 * rank, 2000 + 1000 * rank),
            "v70k": full(25000 * rank, 45000 + 25000 * rank), "w": full(10 * rank, 50 + 10 * rank),
            "s": ["s%04d" % x for x in full(100 * rank, 200 + 100 * rank)]}


def _pin(table, cols):
    import _oracle
    return [table.pin_segment(_oracle.make_segment(SCHEMA, {c: v[i * DOCS:(i + 1) * DOCS] for c, v in cols.items()}))
            for i in range(SEGS_PER_RANK)]


def _combined(table, handles, q, stream, shard, comm):
    """Plan, agree on the mode, execute into the plan's own table, combine, finalize: this rank's share."""
    from pinot_amd.combine import combine_mode, combine_plan
    probe = table.plan(handles, q)
    _, nkeys, _ = probe.layout()
    mode, kinds = combine_mode(probe, comm, 0 if shard else 1 << 62)
    probe.close()
    assert mode == (L.COMBINE_REDUCE_SCATTER if shard else L.COMBINE_ALL_REDUCE), mode
    plan = table.plan_execute(handles, q, stream)
    try:
        k0, kn = combine_plan(plan, comm, stream, mode, kinds)
        groups = plan.finalize(stream).as_dict()
    finally:
        plan.close()
    return {"groups": groups, "range": (k0, kn), "nkeys": nkeys}


def _worker(rank, uid, out_dir):
    from pinot_amd.combine import Communicator, combine_mode, union_dictionaries_comm
    from pinot_amd.executor import GpuTable
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())  # (handle 0 means "the table's own stream" to the C ABI)
    stream = torch.cuda.current_stream().cuda_stream
    comm = Communicator(L.COMM_HOST, uid, WORLD, rank, 0)
    comm.set_timeout(60_000)  # a rank that fails must not leave the other waiting for long
    table = GpuTable(SCHEMA, device=0)
    out = {}
    try:
        handles = _pin(table, _rank_columns(rank))
        union_dictionaries_comm(table, UNIONED, comm)
        out["cards"] = {c: len(table.dictionary(c)) for c in CARDS}
        # a distinct column outside the union: declined on every rank, and the communicator stays usable
        probe = table.plan(handles, parse_query(MISMATCH, num_groups_limit=LIMIT))
        try:
            combine_mode(probe, comm, 1 << 62)
            out["mismatch"] = (0, "no error")
        except L.PinotGpuError as e:
            out["mismatch"] = (e.code, e.message)
        probe.close()
        # ranks that disagree on the dense mode would meet as rows: still declined
        probe = table.plan(handles, parse_query(CASES["all_reduce"][0], num_groups_limit=LIMIT))
        try:
            combine_mode(probe, comm, 0 if rank == 0 else 1 << 62)
            out["disagree"] = ("no error", "")
        except L.PinotGpuError as e:
            out["disagree"] = (type(e).__name__, e.message)
        probe.close()
        for name, (sql, shard) in CASES.items():
            q = parse_query(sql, num_groups_limit=LIMIT)
            out[name] = _combined(table, handles, q, stream, shard, comm)
            if name in AGAIN:
                out[name + "_again"] = _combined(table, handles, q, stream, shard, comm)
        # rank 1 passes a plan it never executed: both ranks fail, at the status exchange before the bitmap all-to-all,
        # and the communicator serves the next query
        from pinot_amd.combine import combine_plan
        q = parse_query(CASES["all_reduce"][0], num_groups_limit=LIMIT)
        probe = table.plan(handles, q)
        mode, kinds = combine_mode(probe, comm, 1 << 62)
        probe.close()
        plan = table.plan(handles, q) if rank == 1 else table.plan_execute(handles, q, stream)
        t0 = time.monotonic()
        try:
            combine_plan(plan, comm, stream, mode, kinds)
            out["failing"] = (0, "no error", time.monotonic() - t0)
        except L.PinotGpuError as e:
            out["failing"] = (e.code, e.message, time.monotonic() - t0)
        plan.close()
        out["after_failure"] = _combined(table, handles, q, stream, False, comm)
    finally:
        with open(os.path.join(out_dir, "rank_%d.pkl" % rank), "wb") as f:
            pickle.dump(out, f)
        table.close()
        comm.close()


@pytest.fixture(scope="module")
def ranks(gpu_lib, tmp_path_factory):
    """The two ranks' dumps (one worker run for the module).  The parent ends the workers past the time limit."""
    from pinot_amd.combine import Communicator
    out_dir = tmp_path_factory.mktemp("distinct_combine")
    uid = Communicator.unique_id(L.COMM_HOST)
    ctx = mp.spawn(_worker, args=(uid, str(out_dir)), nprocs=WORLD, join=False)
    t0, limit_s = time.time(), 150
    while not ctx.join(timeout=2):
        if time.time() - t0 > limit_s:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail("ranks did not finish within %d s" % limit_s)
    return [pickle.load(open(out_dir / ("rank_%d.pkl" % r), "rb")) for r in range(WORLD)]


@pytest.fixture(scope="module")
def docs():
    """Per rank and concatenated value columns (the reference's input)."""
    per_rank = [_rank_columns(r) for r in range(WORLD)]
    allc = {c: (np.concatenate([p[c] for p in per_rank]) if t != "STRING" else sum([p[c] for p in per_rank], []))
            for c, t in SCHEMA}
    return per_rank, allc


def _mask(sql, c):
    if "f < 40" in sql:
        return c["f"] < 40
    if "BETWEEN" in sql:
        return (c["f"] >= 10) & (c["f"] <= 50) & (c["d"] >= 3) & (c["d"] <= 29)
    return np.ones(len(c["f"]), dtype=bool)


def _reference(c, q, mask):
    """{key: [one integer per aggregation]}: DISTINCTCOUNT by set counting, the others by numpy over the group's docs."""
    dcols = [col for fn, col in q.aggregations if fn == "DISTINCTCOUNT"]
    counts = D.distinct_counts([c[g] for g in q.group_by], [c[col] for col in dcols], mask)
    idx = np.nonzero(mask)[0]
    uniq, inv = np.unique(np.stack([c[g][idx] for g in q.group_by], axis=1), axis=0, return_inverse=True)
    order = np.argsort(inv.reshape(-1), kind="stable")
    bounds = np.searchsorted(inv.reshape(-1)[order], np.arange(len(uniq) + 1))
    out = {}
    for gi, key in enumerate(map(tuple, uniq.tolist())):
        sel = idx[order[bounds[gi]:bounds[gi + 1]]]
        row, j = [], 0
        for fn, col in q.aggregations:
            if fn == "DISTINCTCOUNT":
                row.append(counts[key][j])
                j += 1
            else:
                row.append(len(sel) if fn == "COUNT" else int(getattr(c[col][sel], fn.lower())()))
        out[key] = row
    assert set(out) == set(counts)
    return out


def _ints(groups):
    out = {}
    for k, row in groups.items():
        assert all(x == int(x) for x in row), (k, row)
        out[k] = [int(x) for x in row]
    return out


@pytest.fixture(scope="module")
def reference(docs):
    """Each case's expected groups over the docs of both ranks, computed once."""
    _, allc = docs
    return {name: _reference(allc, parse_query(sql, num_groups_limit=LIMIT), _mask(sql, allc))
            for name, (sql, _) in CASES.items()}


def _owned(nkeys, rank):
    chunk = -(-nkeys // WORLD)
    return min(nkeys, rank * chunk), min(nkeys, (rank + 1) * chunk) - min(nkeys, rank * chunk)


def test_data_tells_a_merge_from_a_sum_or_one_rank(docs, reference):
    """On the CPU: for some group the merged count is neither a rank's own count nor the sum of the two."""
    per_rank, _ = docs
    sql = CASES["all_reduce"][0]
    q = parse_query(sql, num_groups_limit=LIMIT)
    own = [_reference(c, q, _mask(sql, c)) for c in per_rank]
    for a in (1, 3):  # DISTINCTCOUNT(v3k), DISTINCTCOUNT(v70k)
        assert any(k in own[0] and k in own[1] and row[a] not in (own[0][k][a], own[1][k][a]) and
                   row[a] != own[0][k][a] + own[1][k][a] for k, row in reference["all_reduce"].items())


def test_union_gives_the_cardinalities_at_the_word_boundaries(ranks):
    for r in ranks:
        assert r["cards"] == CARDS


@pytest.mark.parametrize("name", ["all_reduce", "word_edges", "g1_all_reduce"])
def test_all_reduce_merges_the_sets(ranks, reference, name):
    """Both ranks hold the whole answer: the distinct counts of the union of the ranks' docs, beside the other
    aggregations of the query."""
    exp = reference[name]
    assert len(exp) == (1 if name.startswith("g1") else 41)
    for r in range(WORLD):
        assert ranks[r][name]["range"] == (0, ranks[r][name]["nkeys"])
        assert _ints(ranks[r][name]["groups"]) == exp, (name, r)


@pytest.mark.parametrize("name", ["odd", "g1_reduce_scatter"])
def test_reduce_scatter_leaves_each_rank_its_key_range(ranks, reference, name):
    """shard_bytes = 0: each rank finalizes its own key range; the shares are disjoint and together the reference."""
    exp = reference[name]
    nkeys = ranks[0][name]["nkeys"]
    assert nkeys == (1107 if name == "odd" else 1)
    shares = [_ints(ranks[r][name]["groups"]) for r in range(WORLD)]
    for r in range(WORLD):
        assert ranks[r][name]["nkeys"] == nkeys and ranks[r][name]["range"] == _owned(nkeys, r)
    assert not set(shares[0]) & set(shares[1])
    assert {**shares[0], **shares[1]} == exp
    if name == "odd":
        assert shares[0] and shares[1]
    else:
        assert shares[1] == {} and ranks[1][name]["range"] == (1, 0)  # the second rank owns no key


@pytest.mark.parametrize("name", AGAIN)
def test_reexecution_through_the_plan_cache_combines_again(ranks, name):
    for r in range(WORLD):
        assert ranks[r][name + "_again"] == ranks[r][name] and ranks[r][name]["groups"]


def test_distinct_column_outside_the_union_is_refused_on_every_rank(ranks, reference):
    for r in range(WORLD):
        code, msg = ranks[r]["mismatch"]
        assert code == L.PGPU_ERR_INVALID_ARGUMENT, ranks[r]["mismatch"]
        assert "DISTINCTCOUNT" in msg and "(w)" in msg and "pgpu_table_add_dictionary_values" in msg, msg
        # the communicator was still usable: the cases that followed ran
        assert _ints(ranks[r]["all_reduce"]["groups"]) == reference["all_reduce"]


def test_ranks_that_disagree_on_the_mode_stay_declined(ranks):
    for r in range(WORLD):
        kind, msg = ranks[r]["disagree"]
        assert kind == "UnsupportedQueryError" and "DISTINCTCOUNT" in msg and "rows" in msg, ranks[r]["disagree"]


def test_a_rank_that_fails_its_checks_fails_with_its_peer(ranks, reference):
    """The status exchange before the bitmap all-to-all: rank 1's plan was never executed, rank 0 learns it there
    instead of waiting in the all-to-all; the next query on the same communicator combines."""
    code1, msg1, waited1 = ranks[1]["failing"]
    code0, msg0, waited0 = ranks[0]["failing"]
    assert code1 == L.PGPU_ERR_INVALID_ARGUMENT and "not executed" in msg1, ranks[1]["failing"]
    assert code0 == L.PGPU_ERR_INVALID_ARGUMENT and "rank 1 of 2 failed" in msg0, ranks[0]["failing"]
    assert waited0 < 30 and waited1 < 30
    for r in range(WORLD):
        assert _ints(ranks[r]["after_failure"]["groups"]) == reference["all_reduce"]


@pytest.fixture(scope="module")
def local_table(gpu_lib):
    from pinot_amd.executor import GpuTable
    torch.cuda.set_device(0)
    table = GpuTable(SCHEMA, device=0)
    handles = _pin(table, _rank_columns(0))
    yield table, handles
    table.close()


@pytest.mark.parametrize("shard", [False, True], ids=["all_reduce", "reduce_scatter"])
@pytest.mark.parametrize("kind", ["host", "rccl"])
def test_one_rank_communicator_equals_the_local_answer(local_table, kind, shard):
    """N == 1 passes through the same code (the all-to-all is a copy, the merge an OR of one block) on a one-rank host
    and a one-rank RCCL communicator."""
    from pinot_amd.combine import Communicator
    table, handles = local_table
    k = L.COMM_HOST if kind == "host" else L.COMM_RCCL
    comm = Communicator(k, Communicator.unique_id(k), 1, 0, 0)
    stream = torch.cuda.Stream()
    try:
        for name in ("all_reduce", "odd", "word_edges"):
            q = parse_query(CASES[name][0], num_groups_limit=LIMIT)
            local = table.execute_groupby(handles, q, stream.cuda_stream).as_dict()
            got = _combined(table, handles, q, stream.cuda_stream, shard, comm)
            assert got["range"] == (0, got["nkeys"])
            assert got["groups"] == local and local, name
    finally:
        stream.synchronize()
        comm.close()
