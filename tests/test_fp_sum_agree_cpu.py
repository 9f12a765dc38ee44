"""The cross-rank agreement on the fixed-point format of FLOAT / DOUBLE sums (PGPU_OPT_EXACT_FP_SUM), on the host.

Digit sums of different formats do not add, so before a cross-GPU query every rank reports what its plan could read
(pgpu_query_fp_sum_ranges), the reports are merged (pgpu_fp_sum_ranges_merge: `finite` AND, `any` OR, E max and L min
over the ranks with operands, docs and integer bounds summed) and every rank plans with the result
(pgpu_plan_create_agreed).  Here: the merge against the rule written in Python; the collective form over the host
transport between 2 and 3 CPU processes; and tools/fx_agree_check.cpp, compiled alone under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program -- R synthetic ranks split in the agreed format, digit sums per rank
and across ranks, against a long-integer reference; with every rank in its own format it must fail.  No GPU is touched.
"""
import ctypes
import multiprocessing as mp
import os
import random
import shutil
import subprocess

import pytest

from pinot_amd import _lib as L

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc is needed to build the sanitized check")

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


# ------------------------------------------------------------------------------------------------ the merge rule
def rule(per_rank):
    """The agreement rule on tuples (is_sum, any, finite, E, L, docs, int_sum_bound), one list per rank."""
    out = []
    for a in range(len(per_rank[0])):
        col = [r[a] for r in per_rank]
        if len({bool(c[0]) for c in col}) != 1:
            return None
        if not col[0][0]:
            out.append((0, 0, 0, 0, 0, 0, 0.0))
            continue
        have = [c for c in col if c[1]]
        bound = sum(int(c[6]) for c in col)  # exact: the bounds below are integers
        out.append((1, int(bool(have)), int(all(c[2] for c in col)), max((c[3] for c in have), default=0),
                    min((c[4] for c in have), default=0), sum(c[5] for c in col), float(bound)))
    return out


def random_ranges(rng, nranks, num_aggs):
    kinds = [rng.random() < 0.7 for _ in range(num_aggs)]
    per_rank = []
    for _ in range(nranks):
        row = []
        for is_sum in kinds:
            if not is_sum:
                row.append((0, 0, 0, 0, 0, 0, 0.0))
                continue
            has = rng.random() < 0.8
            e = rng.randint(-1074, 1024)
            # bounds that are powers of two: their sums are exact in a double up to 2^53 x the smallest
            bound = float(2 ** rng.randint(40, 61)) if rng.random() < 0.5 else 0.0
            row.append((1, int(has), int(rng.random() < 0.9), e if has else 0, e - rng.randint(0, 120) if has else 0,
                        rng.randint(0, 10 ** 9), bound))
        per_rank.append(row)
    return per_rank


def merged(per_rank):
    return [r.as_tuple() for r in L.merge_fp_sum_ranges(per_rank)]


@pytest.mark.parametrize("nranks", range(1, 9))
def test_merge_follows_the_rule(nranks):
    rng = random.Random(100 + nranks)
    for _ in range(50):
        per_rank = random_ranges(rng, nranks, rng.randint(1, 6))
        assert merged(per_rank) == rule(per_rank)
        assert merged(per_rank[::-1]) == rule(per_rank)  # the order of the ranks does not matter


def test_merge_of_ranks_without_operands():
    none = (1, 0, 1, 0, 0, 5, 0.0)
    some = (1, 1, 1, -3, -40, 7, 0.0)
    assert merged([[none], [none]]) == [(1, 0, 1, 0, 0, 10, 0.0)]
    # E = 0 / L = 0 of a rank without operands are placeholders: they must not widen the range
    assert merged([[none], [some], [none]]) == [(1, 1, 1, -3, -40, 17, 0.0)]
    assert merged([[some]]) == [some]


def test_one_non_finite_rank_makes_the_agreed_range_non_finite():
    a = (1, 1, 1, 55, 2, 100, 0.0)
    b = (1, 1, 0, 10, -30, 50, 0.0)
    assert merged([[a], [b], [a]]) == [(1, 1, 0, 55, -30, 250, 0.0)]
    assert merged([[a], [a]])[0][2] == 1


def test_integer_bounds_add_up_across_two_to_the_62():
    """Each rank's own bound is below 2^62 (its own plan would keep the int64 slot); together they pass it, and every
    rank must see that -- pgpu_plan_create_agreed compares the agreed bound with 2^62."""
    half = (1, 1, 1, 61, 0, 1000, 2.0 ** 61)
    below = (1, 1, 1, 61, 0, 1000, 2.0 ** 61 - 2.0 ** 9)
    assert merged([[half], [half]])[0][6] == 2.0 ** 62
    assert merged([[below], [half]])[0][6] < 2.0 ** 62
    assert merged([[half], [half], [below]])[0][6] > 2.0 ** 62
    # the sum is rounded up, never down: 2^61 + 1 is not a double
    assert merged([[half], [(1, 1, 1, 1, 0, 1, 1.0)]])[0][6] > 2.0 ** 61


def test_merge_refuses_ranks_that_differ_on_is_sum():
    s = (1, 1, 1, 3, 0, 10, 0.0)
    c = (0, 0, 0, 0, 0, 0, 0.0)
    with pytest.raises(L.PinotGpuError) as e:
        merged([[s, c], [s, s]])
    assert e.value.code == L.PGPU_ERR_INVALID_ARGUMENT and "aggregation 1" in e.value.message
    assert rule([[s, c], [s, s]]) is None


def test_entry_points_validate_their_arguments_without_a_device():
    lib = L.load()
    out = (L.FpSumRangeC * 1)()
    assert lib.pgpu_fp_sum_ranges_merge(None, 2, 1, out) == L.PGPU_ERR_INVALID_ARGUMENT
    assert lib.pgpu_fp_sum_ranges_merge(out, 0, 1, out) == L.PGPU_ERR_INVALID_ARGUMENT
    assert lib.pgpu_query_fp_sum_ranges(None, None, 0, None, out) == L.PGPU_ERR_INVALID_ARGUMENT
    assert lib.pgpu_comm_agree_fp_sum_ranges(None, out, 1) == L.PGPU_ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    assert lib.pgpu_plan_create_agreed(None, None, 0, None, out, ctypes.byref(h)) == L.PGPU_ERR_INVALID_ARGUMENT
    assert ctypes.sizeof(L.FpSumRangeC) == 40


# ------------------------------------------------------------------------------- the collective, host transport
def _mine(rank):
    """Rank `rank`'s report of two aggregations: a SUM whose operands shrink with the rank, and a COUNT."""
    return [(1, 1, 1, 55 - 20 * rank, 2 - 20 * rank, 1000 + rank, float(2 ** (50 + rank))), (0, 0, 0, 0, 0, 0, 0.0)]


def _agree_rank(uid, rank, world, q):
    try:
        from pinot_amd.combine import Communicator, agree_fp_sum_ranges
        c = Communicator(L.COMM_HOST, uid, world, rank, 0)
        c.set_timeout(30000)
        got = agree_fp_sum_ranges([L.FpSumRangeC.from_tuple(t) for t in _mine(rank)], c)
        c.close()
        q.put((rank, [g.as_tuple() for g in got]))
    except Exception as e:  # noqa: BLE001 -- reported to the parent
        q.put((rank, "error: %r" % e))


@pytest.mark.parametrize("world", [2, 3])
def test_agreement_over_the_host_transport(world):
    from pinot_amd.combine import Communicator
    uid = Communicator.unique_id(L.COMM_HOST)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_agree_rank, args=(uid, r, world, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=60) for _ in range(world))
    for p in procs:
        p.join(timeout=30)
    want = rule([_mine(r) for r in range(world)])
    assert want[0][3:5] == (55, 2 - 20 * (world - 1))
    for r in range(world):
        assert out[r] == want, (r, out[r])


# ------------------------------------------------------------------------------------------- the sanitized check
@pytest.fixture(scope="module")
def check():
    from pinot_amd import build
    return build.build_fx_agree_check()


def _run(check, *args):
    res = subprocess.run([check, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=ENV,
                         timeout=300)
    return res.returncode, res.stdout


@needs_hipcc
def test_agreed_format_sums_equal_the_long_integer_reference(check):
    rc, out = _run(check)
    assert rc == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert " 0 failures" in out, out[-2000:]
    import re
    m = re.search(r"(\d+) cases \((\d+) with a rank whose own format differs\)", out)
    assert m and int(m.group(2)) > 50, out[-2000:]


@needs_hipcc
def test_check_fails_when_every_rank_uses_its_own_format(check):
    """The check has teeth: digit sums split in each rank's own (E, K, W) and added all the same do not give the sum."""
    rc, out = _run(check, "--local-formats")
    assert rc == 1, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert "FAIL magnitudes by rank 1 (2 ranks):" in out, out[:4000]
    import re
    m = re.search(r"\((\d+) with a rank whose own format differs\), (\d+) failures", out)
    assert m and 50 < int(m.group(2)) <= int(m.group(1)), out[-2000:]  # only such cases can fail
    assert "[each rank in its own format]" in out
