"""The key range a rank owns in the dense cross-GPU combine (pinot_amd/csrc/key_range.h: owned_key_range), pinned
against plain Python.  The rows of the group table are reduce-scattered by it and the DISTINCTCOUNT side bitmaps are
exchanged and merged by it, so the two must be one split: rank r owns keys [min(G, r * chunk), min(G, (r + 1) * chunk))
with chunk = ceil(G / N).  The header is compiled alone under AddressSanitizer + UndefinedBehaviorSanitizer
(pinot_amd.build.build_key_range_check) and run as a program.  No GPU is touched."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc is needed to build the sanitized check")

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
KEYS = (0, 1, 2, 1107, 2 ** 20 + 1)
RANKS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def ranges():
    """{(G, N): [(chunk, begin, count) per rank]} as the header computes them."""
    from pinot_amd import build
    check = build.build_key_range_check()
    args = [str(x) for g in KEYS for n in RANKS for x in (g, n)]
    res = subprocess.run([check, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=ENV, timeout=120)
    assert res.returncode == 0, res.stdout[-4000:]
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout, res.stdout[-4000:]
    out = {}
    for line in res.stdout.splitlines():
        g, n, r, chunk, begin, count = map(int, line.split())
        out.setdefault((g, n), []).append((chunk, begin, count))
        assert len(out[(g, n)]) == r + 1
    return out


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("g", KEYS)
def test_owned_ranges_equal_the_plain_split(ranges, g, n):
    got = ranges[(g, n)]
    assert len(got) == n
    chunk = -(-g // n)
    for r, (c, begin, count) in enumerate(got):
        assert c == chunk
        assert begin == min(g, r * chunk)
        assert count == min(g, (r + 1) * chunk) - min(g, r * chunk)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("g", KEYS)
def test_owned_ranges_are_ordered_disjoint_and_cover_the_keys(ranges, g, n):
    at = 0
    for _, begin, count in ranges[(g, n)]:
        assert begin == at and count >= 0  # each range starts where the one before ended: ordered and disjoint
        at += count
    assert at == g  # together all keys
