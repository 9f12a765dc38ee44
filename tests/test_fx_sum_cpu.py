"""The fixed-point FLOAT / DOUBLE sum (query option PGPU_OPT_EXACT_FP_SUM) on the host.

The arithmetic -- the format (E, K, W), the split of an operand into W digits of K bits, the conversion of the W digit
sums into one double -- is one header (pinot_amd/csrc/fx_sum.h) shared by the kernels, the plan, the result conversion
and tools/fx_sum_check.cpp, which is compiled alone under AddressSanitizer + UndefinedBehaviorSanitizer
(pinot_amd.build.build_fx_sum_check) and run as a program: split -> int64 digit sums -> conversion against a
2240-bit long-integer reference, over random operands (1 .. 70 001 of them, 2^-30 .. 2^55 and the whole double range,
mixed signs) and adversarial ones (subnormals, +-DBL_MAX / 4, a single value, all zeros, signs that cancel to 0, ties
of the final rounding), in W = 2 exact, W = 3 exact and W = 3 quantised formats, and the worst-case digits for up to
2^31 operands without an int64 overflow.  No GPU is touched.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

from pinot_amd import _lib as L
from pinot_amd.query import FilterContext, Predicate, QueryContext, parse_query

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc is needed to build the sanitized check")

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def check():
    from pinot_amd import build
    return build.build_fx_sum_check()


def _run(check, *args):
    res = subprocess.run([check, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=ENV,
                         timeout=300)
    return res.returncode, res.stdout


@needs_hipcc
def test_fixed_point_sums_equal_the_long_integer_reference(check):
    rc, out = _run(check)
    assert rc == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert " 0 failures" in out, out[-2000:]
    # every kind of format was met
    import re
    m = re.search(r"W=2 exact (\d+), W=3 exact (\d+), W=3 quantised (\d+)", out)
    assert m and all(int(g) > 0 for g in m.groups()), out[-2000:]


@needs_hipcc
def test_check_fails_without_the_headroom_bits(check):
    """The check has teeth: with K = 62 (no headroom for the docs) the digit sums overflow an int64 -- already three
    worst-case digits do -- and the check says so instead of comparing wrapped sums."""
    rc, out = _run(check, "--no-headroom")
    assert rc == 1, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert "int64 overflow of a digit sum" in out, out[:4000]
    assert "FAIL worst case: 3 digits of 2^62 - 1 overflow an int64" in out.splitlines(), out[:6000]


def test_format_getter_validates_its_arguments_without_a_device():
    lib = L.load()
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert lib.pgpu_plan_fp_sum_format(None, 0, out) == L.PGPU_ERR_INVALID_ARGUMENT
    assert "bad arguments" in L.last_error()
    assert list(out) == [7, 7, 7, 7]


def test_option_bit_reaches_the_c_query():
    """QueryContext(exact_fp_sum=True) and parse_query(..., exact_fp_sum=True) set PGPU_OPT_EXACT_FP_SUM (16) and
    nothing else; the default leaves the options word as it was."""
    assert L.OPT_EXACT_FP_SUM == 16
    index = {"d": 0, "m": 1}
    flt = FilterContext.pred(Predicate.range("m", 1, 5))
    for kw, want in (({}, 0), ({"exact_fp_sum": True}, 16)):
        q = QueryContext(["d"], [("SUM", "m")], flt, **kw)
        assert q.to_c(index)[0].options == want
        assert parse_query("SELECT SUM(m) FROM t GROUP BY d", **kw).to_c(index)[0].options == want
    q = QueryContext(["d"], [("SUM", "m")], use_star_tree=False, sql_group_by=True, exact_fp_sum=True)
    q.timing = True
    assert q.to_c(index)[0].options == 1 | 2 | 8 | 16
    q.exact_fp_sum = False  # options are refreshed on every call
    assert q.to_c(index)[0].options == 1 | 2 | 8
