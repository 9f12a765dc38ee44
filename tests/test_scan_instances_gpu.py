"""The six base instances of the fused scan (scan_direct_body.inc: 0 general sparse, 1 dense, 2 dense without gathers, 3
index + scan pair, 4 / 5 register-leaf pure AND with 2- / 4-doc lane batches), every tile split (shift 0, 1, 2) and the
table-word forms (32-bit MIN / MAX, COUNT packed into a SUM's word) at their edges.

Every case asserts where it ran -- Plan.scan_geometry()["variant"], Plan.group_path() and the observed split, log2(plan
tiles / sum ceil(docs / 8192)) -- before it compares, and fails (never skips) when the plan went elsewhere.  Results are
compared with scan_common.groupby_reference, a Python-integer group-by over the value arrays; FLOAT / DOUBLE values are
multiples of 0.25, so every comparison is ==.  numDocsScanned is the reference's match count,
numEntriesScannedInFilter the oracle's (its model of Pinot's iterators).  Which branch of the kernel a crafted wave-tile
takes is the claim of the pattern builders, recounted by brute force here and in test_scan_patterns_cpu.py.

Tile counts follow the device: plans below 2 x CUs tiles are split, so shift 1 needs [CUs, 2 CUs) tiles and shift 0 at
least 2 CUs -- made with one-doc filler segments, whose docs carry keys and values of their own."""
from dataclasses import replace

import numpy as np
import pytest

import scan_common as SC
from pinot_amd.executor import GpuTable
from pinot_amd.query import parse_query
from pinot_amd.segment import SegmentBuffers
from pinot_amd.segment_files import build_inverted_index

pytestmark = pytest.mark.gpu

SPARSE, DENSE, SIMPLE, PAIR, FAST2, FAST4 = 0, 1, 2, 3, 4, 5
GROUPS_LIMIT = 10 ** 9  # no plan here is numGroupsLimit-sensitive


@pytest.fixture(scope="module")
def cus(gpu_lib):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dict_ids(values):
    return np.unique(np.asarray(values), return_inverse=True)[1]


def _with_inverted(seg, column, values):
    c = dict(seg.columns)
    c[column] = replace(c[column], inv_bytes=build_inverted_index(_dict_ids(values), c[column].cardinality))
    return SegmentBuffers(seg.num_docs, c)


class Table:
    """A pinned table with its value arrays: segments in pin order, `cols(handles)` the concatenated columns."""

    def __init__(self, oracle, schema, inverted=()):
        self.oracle, self.schema, self.inverted = oracle, schema, tuple(inverted)
        self.t = GpuTable(schema)
        self.handles, self.segs, self.data = [], [], {}
        self._inv_cache = {}

    def add(self, cols):
        seg = self.oracle.make_segment(self.schema, cols)
        for c in self.inverted:
            if seg.num_docs == 1:  # (the same bytes for every one-doc segment)
                key = (c, 1)
                if key not in self._inv_cache:
                    self._inv_cache[key] = build_inverted_index([0], 1)
                cc = dict(seg.columns)
                cc[c] = replace(cc[c], inv_bytes=self._inv_cache[key])
                seg = SegmentBuffers(1, cc)
            else:
                seg = _with_inverted(seg, c, cols[c])
        h = self.t.pin_segment(seg)
        self.handles.append(h)
        self.segs.append(seg)
        self.data[h] = {n: np.asarray(cols[n]) for n, _ in self.schema}
        return h

    def docs(self, handles):
        return [len(next(iter(self.data[h].values()))) for h in handles]

    def cols(self, handles):
        return {n: np.concatenate([self.data[h][n] for h in handles]) for n, _ in self.schema}

    def oracle_segs(self, handles):
        by = dict(zip(self.handles, self.segs))
        return [by[h] for h in handles]

    def close(self):
        self.t.close()


def run(tb, handles, q, config=None, streamed=False):
    """(as_dict, stats tuple, group path, geometry, observed shift) of q over `handles`."""
    if config:
        tb.t.set_config(**config)
    try:
        if streamed:
            p = tb.t.plan_execute(handles, q)
        else:
            p = tb.t.plan(handles, q)
            p.execute()
        try:
            r = p.finalize()
            geo = p.scan_geometry()
            return r.as_dict(), r.stats.as_tuple(), p.group_path(), geo, SC.observed_shift(geo["tiles"], tb.docs(handles))
        finally:
            p.close()
    finally:
        if config:
            tb.t.reset_config()


def where_it_ran(path, geo, shift):
    return (int(geo["variant"]), path, shift)


def require(ran, variant, path, shift, what=""):
    if ran != (variant, path, shift):
        pytest.fail("%s meant (variant, path, shift) = %s, the plan ran %s" % (what or "the case", (variant, path, shift), ran))


_ORACLE_CACHE = {}


def entries_in_filter(tb, handles, where, cache_key):
    """numEntriesScannedInFilter of the filter over the segments, from the oracle (it depends on the filter alone)."""
    key = (id(tb), cache_key, where)
    if key not in _ORACLE_CACHE:
        q = parse_query("SELECT COUNT(*) FROM t WHERE %s" % where)
        _ORACLE_CACHE[key] = tb.oracle.run_groupby(tb.schema, tb.oracle_segs(handles), q).stats[1]
    return _ORACLE_CACHE[key]


def check(tb, handles, q, mask, got, stats, where=None, cache_key=None):
    """Groups and statistics against the reference (and the oracle's filter entries)."""
    cols = tb.cols(handles)
    exp, matched = SC.groupby_reference(cols, mask, q.group_by, q.aggregations)
    assert set(got) == set(exp)
    assert got == exp
    assert stats[0] == matched and stats[3] == len(mask)
    if where is not None:
        assert stats[1] == entries_in_filter(tb, handles, where, cache_key)
    return exp


# =============================================================================================== 1. the matrix
M_SCHEMA = [("k1", "INT"), ("k2", "INT"), ("h1", "INT"), ("h2", "INT"), ("f", "INT"), ("f2", "INT"), ("a", "INT"),
            ("vi", "INT"), ("vl", "LONG"), ("vd", "DOUBLE")]
M_DATA_DOCS = (3 * SC.TILE_DOCS, SC.TILE_DOCS + 1, 100)  # 3 tiles (the largest), a one-doc tail tile, a lane tail
M_DATA_TILES = 6


def _matrix_data(rng, n, seg):
    """Dictionaries that are the same contiguous ranges in every data segment (what instance 2 needs): every value of
    a range is placed first, the rest is random."""
    def ranged(lo, hi):
        v = rng.integers(lo, hi, n)
        v[:hi - lo] = np.arange(lo, hi)
        return v
    i = np.arange(n)
    return {"k1": ranged(0, 6), "k2": ranged(0, 5), "h1": (i * 7 + seg * 3) % 9000, "h2": (i * 11 + seg) % 9000,  # (7, 11: coprime with 9000)
            "f": ranged(0, 64), "f2": ranged(0, 64), "a": ranged(0, 8), "vi": ranged(-50, 50), "vl": ranged(0, 100),
            "vd": rng.integers(-40, 40, n) * 0.25}


def _matrix_filler(i):
    """One doc that every filter of the matrix matches, with keys (k1 6..7, k2 5, h1 from 9000) and values (vl from
    100, vd from 10) that no data segment holds."""
    return {"k1": [6 + i % 2], "k2": [i % 6], "h1": [9000 + i], "h2": [i % 9000], "f": [0], "f2": [0], "a": [3],
            "vi": [(i * 7) % 100 - 50], "vl": [100 + i % 50], "vd": [10.0 + (i % 16) * 0.25]}


@pytest.fixture(scope="module")
def matrix(oracle, gpu_lib, cus):
    rng = np.random.default_rng(20)
    tb = Table(oracle, M_SCHEMA, inverted=("a",))
    data = [tb.add(_matrix_data(rng, n, s)) for s, n in enumerate(M_DATA_DOCS)]
    fillers = [tb.add(_matrix_filler(i)) for i in range(2 * cus + 8)]
    # shift 2: below CUs tiles; shift 1: [CUs, 2 CUs); shift 0: at least 2 CUs
    sets = {2: data + fillers[:5], 1: data + fillers[:cus + cus // 2 - M_DATA_TILES],
            0: data + fillers[:2 * cus + 8 - M_DATA_TILES]}
    yield tb, sets
    tb.close()


# instance -> (WHERE, its mask over the value arrays, pgpu_config that steers the plan there)
M_INSTANCES = {
    SPARSE: ("f < 2 OR f2 < 1", lambda c: (c["f"] < 2) | (c["f2"] < 1), {}),         # a general program
    DENSE: ("f < 40", lambda c: c["f"] < 40, {}),                                    # estimated 40/64; a DOUBLE sum
    SIMPLE: ("f < 40", lambda c: c["f"] < 40, {}),                                   # ... and integers only
    PAIR: ("a = 3 AND f < 32", lambda c: (c["a"] == 3) & (c["f"] < 32), {}),         # inverted-index leaf AND range leaf
    FAST2: ("f < 2", lambda c: c["f"] < 2, {}),                                      # one leaf, estimated 1/32 < 1/16
    FAST4: ("f < 8", lambda c: c["f"] < 8, {}),                                      # one leaf, 1/16 <= 1/8 < 1/4
}
M_AGGS = "COUNT(*), SUM(vi), MIN(vi), MAX(vi), SUM(vl), SUM(vd), AVG(vd)"
M_AGGS_INT = "COUNT(*), SUM(vi), MIN(vi), MAX(vi), SUM(vl)"  # instance 2 sums no doubles
M_PATHS = {"lds": ("GROUP BY k1, k2", {}), "global": ("GROUP BY k1, k2", {"lds_table_kb": 1}),
           "hash": ("GROUP BY h1, h2", {"hash_partitions": 0}), "g1": ("", {})}
M_CELLS = [(v, p, s) for v in M_INSTANCES for p in M_PATHS for s in (2, 1, 0)
           if not (p == "hash" and v in (DENSE, SIMPLE))]  # a hash table is never scanned by a dense instance


@pytest.mark.parametrize("variant,path,shift", M_CELLS, ids=["v%d-%s-shift%d" % c for c in M_CELLS])
def test_instance_path_shift(matrix, variant, path, shift):
    tb, sets = matrix
    hs = sets[shift]
    where, mask_of, cfg = M_INSTANCES[variant]
    tail, pcfg = M_PATHS[path]
    q = parse_query("SELECT %s FROM t WHERE %s %s" % (M_AGGS_INT if variant == SIMPLE else M_AGGS, where, tail),
                    num_groups_limit=GROUPS_LIMIT)
    got, stats, gpath, geo, s = run(tb, hs, q, {**cfg, **pcfg})
    require(where_it_ran(gpath, geo, s), variant, "lds" if path == "g1" else path, shift)
    if path == "hash":
        assert len(tb.t.dictionary("h1")) * len(tb.t.dictionary("h2")) > 2 ** 26
    cols = tb.cols(hs)
    exp = check(tb, hs, q, mask_of(cols), got, stats, where, shift)
    if path == "g1":
        assert list(exp) == [()]
    else:
        filler_keys = [k for k in exp if (k[0] >= 6 if path != "hash" else k[0] >= 9000)]
        assert filler_keys, "the fillers' own groups are part of the result"


def test_streamed_plan_is_never_the_simple_instance(matrix):
    """stream_chunks = 3: the plan is configured before its later chunks are planned (tile_bound != 0) -- the dense
    instance with gathers even for the integer-only query, three launches, no tile split."""
    tb, sets = matrix
    hs = sets[2]
    cols = tb.cols(hs)
    for aggs in (M_AGGS_INT, M_AGGS):
        q = parse_query("SELECT %s FROM t WHERE f < 40 GROUP BY k1, k2" % aggs, num_groups_limit=GROUPS_LIMIT)
        got, stats, gpath, geo, s = run(tb, hs, q, {"stream_chunks": 3}, streamed=True)
        require(where_it_ran(gpath, geo, s), DENSE, "lds", 0, "the streamed plan")
        check(tb, hs, q, cols["f"] < 40, got, stats, "f < 40", "streamed")
        one, _, _, geo1, s1 = run(tb, hs, q, {"stream_chunks": 1}, streamed=True)
        assert one == got and s1 == 2 and geo1["variant"] == (SIMPLE if aggs == M_AGGS_INT else DENSE)


# =============================================================================================== 2. thresholds
# c: 32 values, c4: 4 values; both are 0 exactly on the crafted matches (estimated 1/32 and 1/4).  a: 3 on the matches
# and on every other doc besides.  k: dictionaries that need a LUT in some segments and an offset in others; k0, vi, vl:
# contiguous in every segment (instance 2).
T_SCHEMA = [("k", "INT"), ("k0", "INT"), ("c", "INT"), ("c4", "INT"), ("a", "INT"), ("vi", "INT"), ("vl", "LONG"),
            ("vd", "DOUBLE")]
T_SIZES = (1, 31, 32, 33, 8191, 8193)
T_CRAFT_DOCS = 3 * SC.TILE_DOCS


def _thresh_cols(match, lut_keys=True):
    n = len(match)
    i = np.arange(n)
    non = (i % 31) + 1
    k = np.array([0, 2, 4, 6, 8, 9])[i % 6] if lut_keys and n >= 6 else i % 10
    return {"k": k, "k0": i % 10, "c": np.where(match, 0, non), "c4": np.where(match, 0, i % 3 + 1),
            "a": np.where(match | (i % 2 == 0), 3, 4), "vi": i % 100 - 50, "vl": i % 100,
            "vd": ((i * 3) % 64 - 32) * 0.25}


def _thresh_filler(j):
    """A filler all of whose docs match: one doc (its dictionaries are one value each: an offset) or two docs whose k
    values are not neighbours in the table's dictionary (a LUT); k0, vi and vl stay contiguous."""
    if j % 2 == 0:
        return {"k": [j % 10], "k0": [j % 10], "c": [0], "c4": [0], "a": [3], "vi": [j % 100 - 50], "vl": [j % 100],
                "vd": [(j % 8) * 0.25]}
    x = j % 8
    return {"k": [x, x + 2], "k0": [x, x + 1], "c": [0, 0], "c4": [0, 0], "a": [3, 3],
            "vi": [j % 99 - 50, j % 99 - 49], "vl": [j % 99, j % 99 + 1], "vd": [0.5, (j % 8) * 0.25]}


def _crafted(shift):
    """The crafted 3-tile segment for a plan split by `shift`: wave-tiles at 255 / 256 / 257 with a neighbour below the
    threshold, lanes at 2 / 3 / 4 / 5, a wave-tile with every doc, and a queue of single matches."""
    last = SC.split_tiles(T_CRAFT_DOCS, shift) - 1
    w = SC.slice_width(shift)
    dense = SC.wave_tile_fill(T_CRAFT_DOCS, shift, {(0, 0): 255, (0, 1): 256, (0, 2): 257, (0, 3): 100,
                                                    (last, 0): 256, (last, 1): 30, (last, 3): SC.WAVE * w})
    lanes = {(1, 0, 5): 2, (1, 0, 9): 2, (1, 1, 7): 3, (1, 1, 8): 2, (1, 2, 0): 4, (1, 2, 63): 4, (1, 3, 1): 5,
             (1, 3, 62): 4}
    lanes.update({(1, 0, l): 1 for l in range(20, 31)})
    return SC.merge_patterns(dense, SC.lane_fill(T_CRAFT_DOCS, shift, lanes))


@pytest.fixture(scope="module")
def thresh(oracle, gpu_lib, cus):
    tb = Table(oracle, T_SCHEMA, inverted=("a",))
    crafted, claims = {}, {}
    for s in (0, 1, 2):
        m, waves, lanes = _crafted(s)
        crafted[s] = tb.add(_thresh_cols(m))
        claims[s] = (m, waves, lanes)
    sizes = [tb.add(_thresh_cols(np.ones(n, dtype=bool))) for n in T_SIZES]
    fillers = [tb.add(_thresh_filler(j)) for j in range(4 * cus + 72)]
    tb.queue_segments = (tb.add(_thresh_cols(QUEUE_A[0])), tb.add(_thresh_cols(QUEUE_B[0])))
    base = 3 + 7  # tiles of a crafted segment and of the size list (8193 docs: 2)
    sets = {2: [crafted[2]] + sizes + fillers[:6], 1: [crafted[1]] + sizes + fillers[:cus + cus // 2 - base],
            0: [crafted[0]] + sizes + fillers[:2 * cus + 8 - base]}
    yield tb, sets, claims, crafted, fillers
    tb.close()


T_AGGS = "COUNT(*), SUM(vi), MIN(vi), MAX(vi), SUM(vl), SUM(vd), AVG(vd)"
T_AGGS_INT = "COUNT(*), SUM(vi), MIN(vi), MAX(vi), SUM(vl)"
# instance -> (query tail, config); every filter matches exactly the docs with c == 0
T_INSTANCES = {
    SPARSE: ("%s FROM t WHERE c = 0 OR c = 77 GROUP BY k" % T_AGGS, "c = 0 OR c = 77", {}),
    DENSE: ("%s FROM t WHERE c = 0 GROUP BY k" % T_AGGS, "c = 0", {"dense_selectivity": 0.0}),
    SIMPLE: ("%s FROM t WHERE c = 0 GROUP BY k0" % T_AGGS_INT, "c = 0", {"dense_selectivity": 0.0}),
    PAIR: ("%s FROM t WHERE a = 3 AND c < 1 GROUP BY k" % T_AGGS, "a = 3 AND c < 1", {}),
    FAST2: ("%s FROM t WHERE c = 0 GROUP BY k" % T_AGGS, "c = 0", {}),
    FAST4: ("%s FROM t WHERE c4 = 0 GROUP BY k" % T_AGGS, "c4 = 0", {"dense_selectivity": 2.0}),
}


@pytest.mark.parametrize("shift", [2, 1, 0])
@pytest.mark.parametrize("variant", sorted(T_INSTANCES))
def test_crafted_thresholds(thresh, variant, shift):
    """The crafted wave-tiles through every instance at every split.  The dense instances decode the wave-tiles of 256
    and 257 matches whole (and the full one, and those of the 8191- and 8193-doc segments, whose last group is
    partial), take 255 in lane batches and 100 and 30 through the queue; the sparse instances batch a wave-tile when a
    lane holds 3 (two batches at 5 in the 4-doc instance, three in the others) and queue it at 2."""
    tb, sets, claims, crafted, _ = thresh
    hs = sets[shift]
    sel, where, cfg = T_INSTANCES[variant]
    q = parse_query("SELECT " + sel, num_groups_limit=GROUPS_LIMIT)
    got, stats, gpath, geo, s = run(tb, hs, q, cfg)
    require(where_it_ran(gpath, geo, s), variant, "lds", shift)
    m, waves, lanes = claims[shift]
    if not SC.check_claims(m, s, waves, lanes):
        pytest.fail("the crafted segment's matches are not where the builders claim at shift %d" % s)
    dense = variant in (DENSE, SIMPLE)
    lane_max = lambda lt, wv: max([n for (a, b, _), n in lanes.items() if (a, b) == (lt, wv)] or [0])
    paths = {k: SC.wave_path(n, lane_max(*k), dense) for k, n in waves.items()}
    last = SC.split_tiles(T_CRAFT_DOCS, s) - 1
    assert paths[(0, 0)] == "batch" and paths[(0, 3)] == paths[(last, 1)] == "queue"  # (100 over 64 lanes: at most 2)
    assert paths[(0, 1)] == paths[(0, 2)] == paths[(last, 0)] == paths[(last, 3)] == ("group" if dense else "batch")
    assert paths[(1, 0)] == "queue" and paths[(1, 1)] == paths[(1, 2)] == paths[(1, 3)] == "batch"
    cols = tb.cols(hs)
    assert (cols["c"] == 0).sum() == (cols["c4"] == 0).sum() == ((cols["a"] == 3) & (cols["c"] < 1)).sum()
    check(tb, hs, q, cols["c"] == 0, got, stats, where, shift)


def _one_tile(lanes_by_wave):
    lanes = {}
    for d in lanes_by_wave:
        lanes.update(d)
    return SC.lane_fill(SC.TILE_DOCS, 0, lanes)


QUEUE_A = _one_tile([SC.queue_fill(0, 0, 1, 127), SC.queue_fill(0, 0, 2, 128), {(0, 3, 11): 3, (0, 3, 12): 1}])
QUEUE_B = _one_tile([SC.queue_fill(0, 0, 1, 128), SC.queue_fill(0, 0, 2, 5), SC.queue_fill(0, 0, 3, 40)])


@pytest.mark.parametrize("variant", [SPARSE, FAST2])
def test_queue_fills_and_the_mixed_final_flush(thresh, cus, variant):
    """More segments than workgroups, so a workgroup's run holds several tiles and its waves' queues live across them.
    Two crafted one-tile segments are put on consecutive tiles of one run (found from the plan's launch geometry with
    scan_common.tile_run): wave 1 queues 127 then 128 matches (drained at 255 of 256), wave 2 exactly 128 (drained at
    the threshold) then 5, wave 3 a lane of 3 (lane batches) then 40.  Wave 0 of most workgroups ends with the single
    matches of several filler segments in its queue: the final flush reads a LUT for some lanes and an offset for
    others."""
    tb, sets, claims, crafted, fillers = thresh
    for pat in (QUEUE_A, QUEUE_B):
        assert SC.check_claims(pat[0], 0, pat[1], pat[2])
    ha, hb = tb.queue_segments
    sel, where, cfg = T_INSTANCES[variant]
    q = parse_query("SELECT " + sel, num_groups_limit=GROUPS_LIMIT)
    first = crafted[0]  # stays first: the plan's selectivity estimate is its first segment's
    with tb.t.plan([first, ha, hb] + fillers, q) as p:
        geo = p.scan_geometry()
    # (launch_* are of the last launch: the plan's own grid and tiles before any)
    grid, tiles = int(geo["grid"]), int(geo["tiles"])
    assert tiles == 3 + 2 + len(fillers) and grid < len(fillers), "more one-doc segments than workgroups: %s" % (geo,)

    def plan_order(chunks):
        runs = [SC.tile_run(b, grid, tiles, chunks) for b in range(grid)]
        pick = next((r for r in runs if len(r) >= 2 and r[0] >= 3), None)
        if pick is None:
            pytest.fail("no workgroup runs two tiles past the first segment: %s" % (geo,))
        order = [None] * (tiles - 3)  # tile t >= 3 is segment t - 3 of the rest (one tile each)
        order[pick[0] - 3], order[pick[1] - 3] = ha, hb
        it = iter(fillers)
        return [first] + [h if h is not None else next(it) for h in order], runs

    # the launch's tile order (chunked or interleaved) is the launch's to say: plan for the first, re-plan if it differs
    chunks = 0
    for attempt in range(2):
        hs, runs = plan_order(chunks)
        got, stats, gpath, geo2, s = run(tb, hs, q, cfg)
        if bool(geo2["tile_chunks"]) == bool(chunks):
            break
        chunks = int(geo2["tile_chunks"])
    require(where_it_ran(gpath, geo2, s), variant, "lds", 0)
    if geo2["slot_weights"] or geo2["launch_grid"] != grid or geo2["launch_tiles"] != tiles or \
            bool(geo2["tile_chunks"]) != bool(chunks):
        pytest.fail("the launch is not the one the segments were ordered for: %s" % (geo2,))
    # the queues of every workgroup and wave, replayed from the segments' matches
    seg_of_tile, per_tile = [], []
    for h in hs:
        mt = tb.data[h]["c"] == 0
        bw, bl = SC.brute_counts(mt, 0)
        for lt in range(bw.shape[0]):
            seg_of_tile.append(h)
            per_tile.append([(int(bw[lt, wv]), int(bl[lt, wv * 64:(wv + 1) * 64].max())) for wv in range(4)])
    assert len(per_tile) == tiles
    drained, finals, mixed = set(), [], 0
    lut_kind = {h: len(tb.data[h]["k"]) == 2 for h in fillers}
    for r in runs:
        for wv in range(4):
            fl, fin = SC.simulate_queue([per_tile[t][wv] for t in r])
            drained.update(fl)
            finals.append(fin)
        tail = [seg_of_tile[t] for t in r if per_tile[t][0][0] and seg_of_tile[t] in lut_kind]
        if len({lut_kind[h] for h in tail}) == 2:
            mixed += 1
    if not {255, 128} <= drained:
        pytest.fail("no queue was drained at 255 and at 128: %s" % sorted(drained))
    if not mixed or max(finals) < 2:
        pytest.fail("no final flush mixes segments with a LUT and with an offset")
    cols = tb.cols(hs)
    check(tb, hs, q, cols["c"] == 0, got, stats, where, "queue-%d" % chunks)


# =============================================================================================== 3. 32-bit MIN / MAX
N_RANGES = {"w0": (0, 2 ** 32 - 2), "w1": (0, 2 ** 32 - 1), "w2": (0, 2 ** 32), "w3": (-1, 100)}
N_SCHEMA = [("g", "INT"), ("c", "INT")] + [(n, "LONG") for n in N_RANGES] + [("wi", "INT")]
N_AGGS = ", ".join("MIN(%s), MAX(%s)" % (n, n) for n in list(N_RANGES) + ["wi"])


def _narrow_cols(rng, match):
    """Groups 0..4: values over the whole range, both ends included; group 5: only the column's maximum; group 6:
    only 0; group 7: no doc matches.  Every group has docs in the dense and in the sparse wave-tiles."""
    n = len(match)
    i = np.arange(n)
    g = np.where(match | (i % 3 != 0), i % 7, 7)  # group 7: only docs that do not match
    cols = {"g": g, "c": np.where(match, 0, i % 5 + 1)}
    for name, (lo, hi) in list(N_RANGES.items()) + [("wi", (0, 2 ** 31 - 1))]:
        v = rng.integers(lo, hi + 1, n, dtype=np.int64)
        for k in range(5):  # both ends among the group's first (dense wave-tiles) and last (sparse) matches
            d = np.flatnonzero(match & (g == k))
            v[d[0]], v[d[1]], v[d[-2]], v[d[-1]] = lo, hi, lo, hi
        v[g == 5] = hi
        v[g == 6] = 0
        d7 = np.flatnonzero(g == 7)
        v[d7[0]], v[d7[1]] = hi, lo  # (the dictionary's ends whatever matches)
        cols[name] = v
    return cols


@pytest.fixture(scope="module")
def narrow(oracle, gpu_lib):
    rng = np.random.default_rng(33)
    tb = Table(oracle, N_SCHEMA)
    # at shift 2: tile 0 dense in waves 0 and 1 (every doc), 40 queued matches in wave 2, lanes of 3 in wave 3
    w = SC.slice_width(2)
    lanes = {(0, 3, l): 3 for l in range(0, 64, 2)}
    lanes.update({(5, 1, l): 2 for l in range(64)})
    m, waves, claimed = SC.merge_patterns(
        SC.wave_tile_fill(2 * SC.TILE_DOCS, 2, {(0, 0): 64 * w, (0, 1): 64 * w, (0, 2): 40, (3, 2): 300, (4, 0): 64 * w}),
        SC.lane_fill(2 * SC.TILE_DOCS, 2, lanes))
    h = tb.add(_narrow_cols(rng, m))
    yield tb, h, (m, waves, claimed)
    tb.close()


def test_narrow_min_max_at_the_32_bit_edges(narrow):
    """Dense LDS plan over LONG columns whose maxima are 2^32 - 2 (32-bit words), 2^32 - 1 and 2^32 (64-bit words: the
    start value of a 32-bit MIN is 2^32 - 1), one with a negative minimum, and an INT column up to 2^31 - 1.  One
    workgroup's waves apply 32-bit atomics (whole-group decode) and 64-bit ones (lane batches, the queue) to the same
    words."""
    tb, h, (m, waves, lanes) = narrow
    q = parse_query("SELECT COUNT(*), %s FROM t WHERE c = 0 GROUP BY g" % N_AGGS)
    got, stats, gpath, geo, s = run(tb, [h], q, {"dense_selectivity": 0.0})
    require(where_it_ran(gpath, geo, s), DENSE, "lds", 2)
    if not SC.check_claims(m, s, waves, lanes):
        pytest.fail("the matches are not where the builders claim")
    assert SC.wave_path(waves[(0, 0)], 8, True) == "group" and SC.wave_path(waves[(0, 2)], 1, True) == "queue"
    assert SC.wave_path(waves[(0, 3)], 3, True) == "batch"
    cols = tb.cols([h])
    mask = cols["c"] == 0
    exp = check(tb, [h], q, mask, got, stats)
    assert sorted(exp) == [(k,) for k in range(7)] and (cols["g"] == 7).any(), "group 7 has docs and none matches"
    for j, (name, (lo, hi)) in enumerate(list(N_RANGES.items()) + [("wi", (0, 2 ** 31 - 1))]):
        assert exp[(5,)][1 + 2 * j] == float(hi) and exp[(6,)][2 + 2 * j] == 0.0  # MIN of the maximum, MAX of 0
        assert exp[(0,)][1 + 2 * j] == float(lo) and exp[(0,)][2 + 2 * j] == float(hi)


def test_narrow_goes_off_for_the_whole_plan(oracle, gpu_lib):
    """The second segment alone holds a negative value: no segment's words may be 32-bit."""
    rng = np.random.default_rng(34)
    tb = Table(oracle, [("g", "INT"), ("c", "INT"), ("w", "LONG")])
    try:
        hs = []
        for seg in range(2):
            n = SC.TILE_DOCS
            g = np.arange(n) % 4
            w = rng.integers(0, 1001, n, dtype=np.int64)
            w[:2] = (0, 1000)
            if seg == 1:
                w[g == 3] = 7   # group 3 of this segment: 7s and one -1
                w[n - 1] = -1
            hs.append(tb.add({"g": g, "c": np.zeros(n, dtype=np.int64) + (np.arange(n) % 64 == 63), "w": w}))
        q = parse_query("SELECT COUNT(*), MIN(w), MAX(w), SUM(w) FROM t WHERE c = 0 GROUP BY g")
        for handles in (hs, hs[:1], hs[1:]):
            got, stats, gpath, geo, s = run(tb, handles, q, {"dense_selectivity": 0.0})
            if gpath != "lds" or s != 2 or geo["variant"] not in (DENSE, SIMPLE):
                pytest.fail("not a dense LDS plan at shift 2: %s" % ((gpath, s, geo),))
            cols = tb.cols(handles)
            check(tb, handles, q, cols["c"] == 0, got, stats)
        q = parse_query("SELECT COUNT(*), MIN(w), MAX(w) FROM t GROUP BY g")  # every doc: the -1 itself
        got, stats, gpath, geo, s = run(tb, hs, q)
        assert gpath == "lds" and geo["variant"] in (DENSE, SIMPLE)
        exp = check(tb, hs, q, np.ones(2 * SC.TILE_DOCS, dtype=bool), got, stats)
        assert exp[(3,)][1] == -1.0
    finally:
        tb.close()


# =============================================================================================== 4. packed COUNT
@pytest.mark.parametrize("k", range(20, 37))
def test_packed_count_lds(oracle, gpu_lib, k):
    """Every doc of a workgroup in one group with the constant value hi = 2^k - 1, 2^k: the sum of a workgroup crosses
    2^40, the COUNT's first bit in a packed word, inside the sweep, wherever the planner stops packing.  Dense (whole
    groups), sparse (lane batches), and with a second group of one doc."""
    docs = 3 * SC.TILE_DOCS
    for hi in (2 ** k - 1, 2 ** k):
        tb = Table(oracle, [("g", "INT"), ("c", "INT"), ("v", "LONG")])
        try:
            g = np.zeros(docs, dtype=np.int64)
            lone = g.copy()
            lone[docs // 2] = 1
            c = np.arange(docs) % 2  # every other doc matches c = 0: 4 per lane slice at shift 2 (lane batches)
            h_all = tb.add({"g": g, "c": c, "v": np.full(docs, hi, dtype=np.int64)})
            h_two = tb.add({"g": lone, "c": np.zeros(docs, dtype=np.int64), "v": np.full(docs, hi, dtype=np.int64)})
            for handles, where, cfg, variant in (([h_all], None, {}, SIMPLE), ([h_all], "c = 0", {"dense_selectivity": 2.0}, FAST4),
                                                 ([h_two], None, {}, SIMPLE), ([h_two], "c = 0", {"dense_selectivity": 2.0}, FAST4)):
                q = parse_query("SELECT COUNT(*), SUM(v) FROM t %s GROUP BY g" % ("WHERE " + where if where else ""))
                got, stats, gpath, geo, s = run(tb, handles, q, cfg)
                require(where_it_ran(gpath, geo, s), variant, "lds", 2, "hi = %d" % hi)
                cols = tb.cols(handles)
                mask = cols["c"] == 0 if where else np.ones(docs, dtype=bool)
                exp = check(tb, handles, q, mask, got, stats)
                n0 = int((mask & (cols["g"] == 0)).sum())
                assert exp[(0,)] == [n0, float(n0 * hi)]
                if handles == [h_two]:
                    assert exp[(1,)] == [1, float(hi)]
        finally:
            tb.close()


@pytest.mark.parametrize("k", range(20, 37))
def test_packed_count_hash(oracle, gpu_lib, k):
    """MODE_HASH (two 9000-value key columns: past 2^26 keys): 11 000 of 19 999 docs in one group with the value hi; the
    COUNT takes the top bits(total docs) bits of the word and hash_unpack splits the words after the scan."""
    for hi in (2 ** k - 1, 2 ** k):
        tb = Table(oracle, [("h1", "INT"), ("h2", "INT"), ("v", "LONG")])
        try:
            j = np.arange(1, 9000)
            h1 = np.concatenate([np.zeros(11000, dtype=np.int64), j])
            h2 = np.concatenate([np.zeros(11000, dtype=np.int64), j[::-1]])
            v = np.concatenate([np.full(11000, hi, dtype=np.int64), j % 7])
            h = tb.add({"h1": h1, "h2": h2, "v": v})
            q = parse_query("SELECT COUNT(*), SUM(v) FROM t GROUP BY h1, h2", num_groups_limit=GROUPS_LIMIT)
            got, stats, gpath, geo, s = run(tb, [h], q, {"hash_partitions": 0})
            require(where_it_ran(gpath, geo, s), SPARSE, "hash", 2, "hi = %d" % hi)
            assert len(tb.t.dictionary("h1")) * len(tb.t.dictionary("h2")) > 2 ** 26
            exp = check(tb, [h], q, np.ones(len(v), dtype=bool), got, stats)
            assert exp[(0, 0)] == [11000, float(11000 * hi)] and len(exp) == 9000
        finally:
            tb.close()


# =============================================================================================== 5. LEAP2
L_SCHEMA = [("g", "INT"), ("a", "INT"), ("b", "INT"), ("vi", "INT")]
A_ONLY, B_ONLY, BOTH = "a", "b", "ab"
KINDS = (A_ONLY, B_ONLY, BOTH)


def _leap_cols(n, places):
    """places: {(lt, wave, lane, bit): kind} at shift 0.  a / b are 1 where the leaf matches, 0 or 2 elsewhere."""
    i = np.arange(n)
    a, b = (i % 2) * 2, ((i // 2) % 2) * 2
    for (lt, wave, lane, bit), kind in places.items():
        d = SC.doc_of(0, lt, wave, lane, bit)
        assert d < n
        if kind in (A_ONLY, BOTH):
            a[d] = 1
        if kind in (B_ONLY, BOTH):
            b[d] = 1
    return {"g": i % 5, "a": a, "b": b, "vi": i % 41 - 20}


def _leap_segment(last0, first1, first0, last1):
    """A two-tile segment: its first match (wave 0, lane 0, bit 0) of kind first0; a wave whose only matches are at
    lane 63; a matchless wave 2; tile 0's last match (wave 3, lane 63, bit 31) of kind last0 followed by tile 1's
    first match of kind first1; in tile 1 a matchless wave 1 between two waves with matches, and the segment's last
    match of kind last1 (wave 2, lane 40)."""
    return {(0, 0, 0, 0): first0, (0, 0, 0, 9): BOTH, (0, 1, 63, 3): B_ONLY, (0, 1, 63, 30): A_ONLY,
            (0, 3, 7, 7): BOTH, (0, 3, 63, 31): last0,
            (1, 0, 0, 0): first1, (1, 0, 33, 2): A_ONLY, (1, 2, 0, 31): B_ONLY, (1, 2, 40, 12): last1}


def test_leap2_entry_counts_at_crafted_boundaries(oracle, gpu_lib):
    """An AND of two scans (leap-frog statistics, one byte per (tile, wave) chained by leap2_compose_kernel): the only
    matches of a wave at lane 0 / lane 63, matchless waves between matching ones, and the last match of a tile being
    A-only, B-only or both before a first match of each kind -- in the next tile and in the next segment."""
    tb = Table(oracle, L_SCHEMA)
    try:
        hs = []
        combos = [(x, y) for x in KINDS for y in KINDS]
        for j in range(10):
            # the segment boundary j -> j + 1 pairs last1 of j with first0 of j + 1: all nine pairs again
            x, y = combos[j % 9]
            hs.append(tb.add(_leap_cols(2 * SC.TILE_DOCS, _leap_segment(x, y, first0=KINDS[j % 3], last1=KINDS[(j // 3) % 3]))))
        pairs = set()
        for j in range(9):
            pairs.add((KINDS[(j // 3) % 3], KINDS[(j + 1) % 3]))
        assert len(pairs) == 9, "every (last of a segment, first of the next) pair of kinds"
        # tails: 1, 31, 33 and 8193 docs, and a random segment
        for n in (1, 31, 33, SC.TILE_DOCS + 1):
            hs.append(tb.add(_leap_cols(n, {(0, 0, 0, 0): BOTH} if n == 1 else {(0, 0, 0, 30): A_ONLY, (0, 0, 0, 2): B_ONLY})))
        rng = np.random.default_rng(55)
        n = 3 * SC.TILE_DOCS
        hs.append(tb.add({"g": rng.integers(0, 5, n), "a": rng.integers(0, 3, n), "b": rng.integers(0, 3, n),
                          "vi": rng.integers(-20, 21, n)}))
        where = "a = 1 AND b = 1"
        q = parse_query("SELECT COUNT(*), SUM(vi), MIN(vi), MAX(vi) FROM t WHERE %s GROUP BY g" % where)
        got, stats, gpath, geo, s = run(tb, hs, q)
        if geo["leap_tiles"] <= 0:
            pytest.fail("the plan keeps no leap-frog statistics: %s" % (geo,))
        require(where_it_ran(gpath, geo, s), FAST4, "lds", 0, "the two-scan AND (never split)")
        cols = tb.cols(hs)
        check(tb, hs, q, (cols["a"] == 1) & (cols["b"] == 1), got, stats)
        o = oracle.run_groupby(L_SCHEMA, tb.oracle_segs(hs), q)
        assert stats == tuple(o.stats)
        # segment by segment: a wrong chain across one boundary is not hidden by the others
        for h in hs:
            r = tb.t.execute_groupby([h], q)
            o1 = oracle.run_groupby(L_SCHEMA, tb.oracle_segs([h]), q)
            assert r.stats.as_tuple() == tuple(o1.stats), "segment %d" % hs.index(h)
    finally:
        tb.close()
