"""The pattern builders of scan_common.py, on the CPU: what each claims about its matches per (tile, wave) and per lane is
recounted by brute force from the doc array (brute_counts derives a doc's place from its number; the builders go the
other way, from a place to its doc).  The GPU tests (test_scan_instances_gpu.py) rely on these claims to say which
branch of the scan kernel a wave-tile takes."""
import numpy as np
import pytest

import scan_common as SC

SHIFTS = (0, 1, 2)
DOCS = 3 * SC.TILE_DOCS  # the largest data segment of the GPU tests


@pytest.mark.parametrize("shift", SHIFTS)
def test_doc_of_covers_every_doc_once(shift):
    """(lt, wave, lane, k) -> doc is a bijection onto the docs of the segment, and split tile lt holds bits
    [w (lt mod 2^shift), +w) of groups (lt >> shift) 256 + tid."""
    w = SC.slice_width(shift)
    seen = np.zeros(DOCS, dtype=np.int64)
    for lt in range(SC.split_tiles(DOCS, shift)):
        for wave in range(4):
            for lane in range(64):
                d0 = SC.doc_of(shift, lt, wave, lane, 0)
                assert d0 // 32 == (lt >> shift) * 256 + wave * 64 + lane
                assert d0 % 32 == w * (lt % (1 << shift))
                seen[d0:d0 + w] += 1
                assert SC.doc_of(shift, lt, wave, lane, w - 1) == d0 + w - 1
    assert (seen == 1).all()


@pytest.mark.parametrize("shift", SHIFTS)
def test_brute_counts_of_a_full_and_a_partial_segment(shift):
    for n in (1, 31, 32, 33, 8191, 8193):
        waves, lanes = SC.brute_counts(np.ones(n, dtype=bool), shift)
        assert waves.shape == (SC.split_tiles(n, shift), 4) and waves.sum() == n == lanes.sum()
        assert lanes.max() == min(n, SC.slice_width(shift))
    waves, _ = SC.brute_counts(np.ones(8193, dtype=bool), shift)
    # the 8193rd doc: bit 0 of thread 0 of the second tile's first split
    assert waves[1 << shift, 0] == 1 and waves[(1 << shift):].sum() == 1


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [255, 256, 257])
def test_wave_tile_at_the_whole_group_threshold(shift, n):
    """255 / 256 / 257 matches in one wave-tile, a neighbour of the same tile below the threshold, the rest empty."""
    last = SC.split_tiles(DOCS, shift) - 1
    fills = {(0, 1): n, (0, 2): 100, (last, 3): n, (last, 0): 17}
    m, waves, lanes = SC.wave_tile_fill(DOCS, shift, fills)
    assert waves == fills and int(m.sum()) == 2 * n + 117
    assert SC.check_claims(m, shift, waves, lanes)
    bw, bl = SC.brute_counts(m, shift)
    assert bw[0, 1] == n and bw[0, 2] == 100 and bw[last, 3] == n and bw[last, 0] == 17 and bw.sum() == 2 * n + 117
    # dealt in turn: no lane is more than one match ahead of another
    per_lane = bl[0, 64:128]
    assert per_lane.max() - per_lane.min() <= 1 and per_lane.max() == -(-n // 64)
    assert (SC.wave_path(n, int(per_lane.max()), dense=True) == "group") == (n >= SC.DENSE_GROUP_MIN)
    assert SC.wave_path(n, int(per_lane.max()), dense=False) == "batch"


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [2, 3, 4, 5])
@pytest.mark.parametrize("spread", [False, True])
def test_lane_at_the_batch_thresholds(shift, n, spread):
    """Exactly n matches in one lane (2 against 3: queue or lane batches; 4 against 5: one 4-doc batch or two), and
    every other lane of the wave-tile at most 1."""
    spread = spread and 2 * n - 1 <= SC.slice_width(shift)  # (5 spread matches need 9 bits: not at shift 2)
    lanes = {(1, 2, 63): n, (1, 2, 0): 1, (1, 2, 17): 1, (1, 3, 5): 2}
    m, waves, claimed = SC.lane_fill(DOCS, shift, lanes, spread=spread)
    assert SC.check_claims(m, shift, waves, claimed)
    bw, bl = SC.brute_counts(m, shift)
    assert bl[1, 2 * 64 + 63] == n and bl[1, 2 * 64:3 * 64].max() == n and bw[1, 2] == n + 2
    assert bl[1, 3 * 64:].max() == 2 and bw[1, 3] == 2
    assert SC.wave_path(int(bw[1, 2]), n, dense=False) == ("queue" if n <= 2 else "batch")
    assert SC.wave_path(int(bw[1, 3]), 2, dense=True) == "queue"
    if spread and n > 1:
        docs = np.flatnonzero(m[SC.doc_of(shift, 1, 2, 63, 0):][:SC.slice_width(shift)])
        assert (np.diff(docs) == 2).all()


@pytest.mark.parametrize("shift", SHIFTS)
def test_queue_fill_sequences(shift):
    """127 then 128 (the queue is drained at 255, one short of its capacity), exactly 128 (drained at the threshold
    itself), and 127 alone (the final flush)."""
    lanes = {}
    lanes.update(SC.queue_fill(shift, 0, 1, 127))
    lanes.update(SC.queue_fill(shift, 1, 1, 128))
    lanes.update(SC.queue_fill(shift, 0, 2, 128))
    lanes.update(SC.queue_fill(shift, 1, 2, 5))
    lanes.update(SC.queue_fill(shift, 1, 3, 127))
    m, waves, claimed = SC.lane_fill(DOCS, shift, lanes)
    assert SC.check_claims(m, shift, waves, claimed)
    bw, bl = SC.brute_counts(m, shift)
    assert bl.max() == 2
    assert [int(bw[t, 1]) for t in (0, 1)] == [127, 128] and [int(bw[t, 2]) for t in (0, 1)] == [128, 5]
    seq = lambda wave: [(int(bw[t, wave]), int(bl[t, wave * 64:(wave + 1) * 64].max())) for t in (0, 1)]
    assert SC.simulate_queue(seq(1)) == ([255], 0)
    assert SC.simulate_queue(seq(2)) == ([128], 5)
    assert SC.simulate_queue(seq(3)) == ([], 127)
    assert SC.simulate_queue(seq(0)) == ([], 0)
    # a lane of 3 takes the wave-tile off the queue
    assert SC.simulate_queue([(127, 2), (3, 3), (1, 1)]) == ([128], 0)
    # the dense instances decode a wave-tile of 256 whole: it never reaches the queue
    assert SC.simulate_queue([(100, 2), (256, 8), (27, 1)], dense=True) == ([], 127)


def test_merge_patterns_and_bounds():
    a = SC.wave_tile_fill(DOCS, 2, {(1, 0): 300})
    b = SC.lane_fill(DOCS, 2, {(1, 1, 7): 3})
    m, waves, lanes = SC.merge_patterns(a, b)
    assert int(m.sum()) == 303 and SC.check_claims(m, 2, waves, lanes)
    with pytest.raises(AssertionError):
        SC.wave_tile_fill(DOCS, 2, {(0, 0): 513})  # a wave-tile at shift 2 holds 512 docs
    with pytest.raises(AssertionError):
        SC.place(100, 0, [(0, 0, 4, 0)])  # doc 128 of a 100-doc segment
    assert not SC.check_claims(m, 1, waves, lanes)  # the same docs are other places at another shift


@pytest.mark.parametrize("grid,tiles,chunks", [(7, 7, 0), (12, 30, 0), (64, 64, 0), (256, 600, 0), (256, 600, 1),
                                               (1024, 1100, 0), (1024, 1100, 1), (512, 515, 1)])
def test_tile_run_partitions_the_tiles(grid, tiles, chunks):
    seen = sorted(t for b in range(grid) for t in SC.tile_run(b, grid, tiles, chunks))
    assert seen == list(range(tiles))


def test_reference_groupby():
    cols = {"k": np.array([1, 1, 2, 2, 2]), "v": np.array([5, -7, 3, 2 ** 40, 1]), "d": np.array([0.25, 0.5, 1.0, 2.0, 4.0])}
    aggs = [("COUNT", "*"), ("SUM", "v"), ("MIN", "v"), ("MAX", "v"), ("AVG", "d")]
    got, n = SC.groupby_reference(cols, np.array([1, 1, 1, 1, 0], dtype=bool), ["k"], aggs)
    assert n == 4
    assert got == {(1,): [2, -2.0, -7.0, 5.0, SC.AvgPair(0.75, 2)], (2,): [2, float(2 ** 40 + 3), 3.0, float(2 ** 40), SC.AvgPair(3.0, 2)]}
    only, n = SC.groupby_reference(cols, np.ones(5, dtype=bool), [], [("SUM", "v"), ("COUNT", "*")])
    assert only == {(): [float(2 ** 40 + 2), 5]} and n == 5
    assert SC.groupby_reference(cols, np.zeros(5, dtype=bool), ["k"], aggs) == ({}, 0)
    assert SC.observed_shift(12, [8193, 1]) == 2 and SC.observed_shift(3, [8193, 1]) == 0
    assert SC.observed_shift(5, [8193, 1]) is None
