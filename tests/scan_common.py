"""Pattern builders and a reference for the tests of the fused scan's instances (test_scan_instances_gpu.py; the
builders themselves are checked on the CPU by test_scan_patterns_cpu.py).

Geometry (scan_direct_body.inc): a segment is cut into tiles of 8192 docs = 256 groups of 32 consecutive docs; thread
`tid` of the workgroup (wave tid >> 6, lane tid & 63) owns group tile * 256 + tid.  A plan of few tiles splits every tile
into 2^shift (split_small_tiles): split tile `lt` of a segment covers bits [w * (lt mod 2^shift), +w), w = 32 >> shift, of
the groups (lt >> shift) * 256 + tid.  A "wave-tile" is what one wave sees of one (split) tile: 64 lanes x w docs.

The reference is a plain Python / numpy group-by, independent of the C oracle: the filter is evaluated on the value
arrays by the caller (a boolean mask), keys are tuples, and COUNT / SUM / MIN / MAX / AVG are computed with Python
integers (floats for FLOAT / DOUBLE columns, whose test values are multiples of 0.25: every summation order is exact)."""
import numpy as np

from pinot_amd.executor import AvgPair

TILE_DOCS = 8192
GROUP_DOCS = 32
BLOCK = 256          # kBlock
WAVE = 64
DENSE_GROUP_MIN = 256  # kDenseGroupMin: matches of a wave-tile from which the dense instances decode whole groups
FLUSH_AT = 128         # kFlushAt: fill at which a wave's queue of sparse matches is drained
WAVE_Q = 256           # kWaveQ: the queue's capacity


# ------------------------------------------------------------------------------------------------ positions
def slice_width(shift):
    return GROUP_DOCS >> shift


def split_tiles(num_docs, shift):
    """Split tiles of a segment of num_docs docs."""
    return ((num_docs + TILE_DOCS - 1) // TILE_DOCS) << shift


def doc_of(shift, lt, wave, lane, k):
    """The doc at bit k (< 32 >> shift) of lane `lane` of wave `wave` in split tile `lt` of its segment."""
    w = slice_width(shift)
    assert 0 <= wave < BLOCK // WAVE and 0 <= lane < WAVE and 0 <= k < w
    group = (lt >> shift) * BLOCK + wave * WAVE + lane
    return group * GROUP_DOCS + w * (lt & ((1 << shift) - 1)) + k


def place(num_docs, shift, positions):
    """A boolean match column of num_docs docs with matches exactly at `positions`, (lt, wave, lane, k) tuples."""
    m = np.zeros(num_docs, dtype=bool)
    for lt, wave, lane, k in positions:
        d = doc_of(shift, lt, wave, lane, k)
        assert d < num_docs, "position (%d, %d, %d, %d) is doc %d, past the segment's %d" % (lt, wave, lane, k, d, num_docs)
        assert not m[d], "position placed twice"
        m[d] = True
    return m


def brute_counts(match, shift):
    """By brute force over the doc array: (matches per (split tile, wave) [tiles, 4], per (split tile, thread)
    [tiles, 256]).  Walks the docs in order and derives each doc's place from its number alone (not from doc_of)."""
    n = len(match)
    tiles = split_tiles(n, shift)
    lanes = np.zeros((max(tiles, 1), BLOCK), dtype=np.int64)
    per_slice = GROUP_DOCS >> shift
    for d in np.flatnonzero(np.asarray(match, dtype=bool)).tolist():
        base_tile, in_tile = divmod(d, TILE_DOCS)
        tid, bit = divmod(in_tile, GROUP_DOCS)
        sub = bit // per_slice
        lanes[base_tile * (1 << shift) + sub, tid] += 1
    waves = lanes.reshape(lanes.shape[0], BLOCK // WAVE, WAVE).sum(axis=2)
    return waves, lanes


# ------------------------------------------------------------------------------------------------ builders
# Each returns (match column, claimed {(lt, wave): matches}, claimed {(lt, wave, lane): matches}); wave-tiles and lanes
# that are not named hold no match.
def wave_tile_fill(num_docs, shift, fills):
    """fills: {(lt, wave): n} -- n matches in that wave-tile, dealt to the lanes in turn (match i at lane i mod 64, bit
    i div 64), so the lanes hold n div 64 or one more."""
    w = slice_width(shift)
    pos, lanes = [], {}
    for (lt, wave), n in fills.items():
        assert 0 <= n <= WAVE * w, "a wave-tile at shift %d holds %d docs" % (shift, WAVE * w)
        for i in range(n):
            pos.append((lt, wave, i % WAVE, i // WAVE))
            lanes[(lt, wave, i % WAVE)] = lanes.get((lt, wave, i % WAVE), 0) + 1
    return place(num_docs, shift, pos), {k: v for k, v in fills.items() if v}, lanes


def lane_fill(num_docs, shift, lanes, spread=False):
    """lanes: {(lt, wave, lane): n} -- n matches in that lane's slice of the tile; the lowest bits, or (spread) every
    other bit from the top, so the matches are not adjacent."""
    w = slice_width(shift)
    pos, waves = [], {}
    for (lt, wave, lane), n in lanes.items():
        assert 0 <= n <= (w if not spread else (w + 1) // 2)
        for i in range(n):
            pos.append((lt, wave, lane, i if not spread else w - 1 - 2 * i))
        if n:
            waves[(lt, wave)] = waves.get((lt, wave), 0) + n
    return place(num_docs, shift, pos), waves, {k: v for k, v in lanes.items() if v}


def merge_patterns(*patterns):
    """The union of patterns over one segment (their named wave-tiles must be disjoint)."""
    m = np.zeros_like(patterns[0][0])
    waves, lanes = {}, {}
    for pm, pw, pl in patterns:
        assert not (m & pm).any() and not (set(waves) & set(pw))
        m |= pm
        waves.update(pw)
        lanes.update(pl)
    return m, waves, lanes


def queue_fill(shift, lt, wave, n):
    """{(lt, wave, lane): 1 or 2}: n <= 128 matches of a wave-tile with at most 2 in any lane (the queue path:
    no lane holds more than 2), every lane 1 before any lane 2."""
    assert 0 <= n <= 2 * WAVE and slice_width(shift) >= 2
    return {(lt, wave, lane): 1 + (1 if lane + WAVE < n else 0) for lane in range(min(n, WAVE))}


def check_claims(match, shift, waves, lanes):
    """The claimed counts against brute_counts: every named wave-tile / lane holds what is claimed, the others nothing."""
    bw, bl = brute_counts(match, shift)
    exp_w = np.zeros_like(bw)
    for (lt, wave), n in waves.items():
        exp_w[lt, wave] = n
    exp_l = np.zeros_like(bl)
    for (lt, wave, lane), n in lanes.items():
        exp_l[lt, wave * WAVE + lane] = n
    return bool((bw == exp_w).all() and (bl == exp_l).all())


# ------------------------------------------------------------------------------------------------ the kernel's choices
def tile_run(block, grid, tiles, tile_chunks):
    """tile_split (tile_split.h) for equal shares: the tiles of workgroup `block` of `grid` in a launch of `tiles`."""
    if grid >= 64 and grid % 8 == 0 and tile_chunks:
        x, i, nx = block & 7, block >> 3, grid >> 3
        lo = x * tiles // 8
        ln = (x + 1) * tiles // 8 - lo
        return list(range(lo + i * ln // nx, lo + (i + 1) * ln // nx))
    if grid >= 64 and grid % 8 == 0:
        x = block & 7
        return list(range(x * tiles // 8 + (block >> 3), (x + 1) * tiles // 8, grid >> 3))
    return list(range(block * tiles // grid, (block + 1) * tiles // grid))


def wave_path(count, lane_max, dense):
    """What a wave does with a wave-tile of `count` matches, at most `lane_max` in a lane: "group" (whole-group decode,
    dense instances), "batch" (lane batches: some lane holds more than 2), "queue" or "none"."""
    if dense and count >= DENSE_GROUP_MIN:
        return "group"
    if lane_max > 2:
        return "batch"
    return "queue" if count else "none"


def simulate_queue(wave_tiles, dense=False):
    """wave_tiles: the (count, lane_max) of one wave over the tiles of its workgroup's run, in order.  Returns the
    fills at which the queue was drained inside the loop, and the fill of the final flush (0: none)."""
    qn, flushes = 0, []
    for count, lane_max in wave_tiles:
        if wave_path(count, lane_max, dense) != "queue":
            continue
        qn += count
        assert qn <= WAVE_Q
        if qn >= FLUSH_AT:
            flushes.append(qn)
            qn = 0
    return flushes, qn


# ------------------------------------------------------------------------------------------------ reference
def _is_float(a):
    return np.asarray(a).dtype.kind == "f"


def groupby_reference(columns, mask, group_by, aggregations):
    """{key tuple: [results]} over the docs of `mask`: columns name -> value array (all segments concatenated),
    aggregations [(fn, column)].  Results as the executor decodes them: COUNT an int, SUM / MIN / MAX a float (of an
    exactly computed Python integer for integer columns), AVG an AvgPair; the empty tuple keys an aggregation-only
    query.  Also returns the match count (numDocsScanned)."""
    docs = np.flatnonzero(np.asarray(mask, dtype=bool))
    keycols = [np.asarray(columns[c])[docs].tolist() for c in group_by]
    groups = {}
    for j, d in enumerate(docs.tolist()):
        groups.setdefault(tuple(kc[j] for kc in keycols), []).append(d)
    vals = {}
    for fn, c in aggregations:
        if c != "*" and c not in vals:
            a = np.asarray(columns[c])
            vals[c] = (a.tolist(), _is_float(a))  # Python ints / floats
    out = {}
    for k, ds in groups.items():
        row = []
        for fn, c in aggregations:
            if fn == "COUNT":
                row.append(len(ds))
                continue
            v, _ = vals[c]
            x = [v[d] for d in ds]
            if fn == "SUM":
                row.append(float(sum(x)))
            elif fn == "MIN":
                row.append(float(min(x)))
            elif fn == "MAX":
                row.append(float(max(x)))
            elif fn == "AVG":
                row.append(AvgPair(float(sum(x)), len(x)))
            else:
                raise ValueError(fn)
            if fn in ("SUM", "AVG"):
                s = sum(x)
                assert abs(s) < 2 ** 53 and float(s) == s, "the expected sum is not exact in a double"
        out[k] = row
    return out, int(len(docs))


def observed_shift(geometry_tiles, seg_docs):
    """log2(plan tiles / sum ceil(n / 8192)); None when the ratio is no power of two."""
    base = sum((n + TILE_DOCS - 1) // TILE_DOCS for n in seg_docs)
    for s in range(3):
        if base << s == geometry_tiles:
            return s
    return None
