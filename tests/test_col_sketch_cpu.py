"""The byte-code sketches of filter columns on the host (tools/col_sketch_check.cpp).

A sketch maps a segment's dictIds to at most 256 codes, monotone in the dictId: up to 127 of the most frequent dictIds
get a code of their own, the dictIds between them share interval codes (pinot_amd/csrc/col_sketch.h).  The planner scans
the 8-bit codes instead of the dictIds only for the predicates the codes answer exactly, so the assignment and the two
exactness tests are what keeps results bit for bit.  They are one header shared by the pin-time builder, the planner and
this check, which is compiled alone under AddressSanitizer + UndefinedBehaviorSanitizer
(pinot_amd.build.build_col_sketch_check) and run as a program over random and adversarial histograms: cardinalities 1,
255, 256, 257, 2049 and 100 000; all counts equal; all mass on the first / last dictId; adjacent hot ids; more than 127
tied candidates; zero-count ids.  No GPU is touched.
"""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc is needed to build the sanitized check")

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def check():
    from pinot_amd import build
    return build.build_col_sketch_check()


def test_assignment_and_exactness(check):
    res = subprocess.run([check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=ENV, timeout=300)
    out = res.stdout
    assert res.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert " 0 failures" in out, out[-2000:]
    cases = re.search(r"(\d+) range / set cases", out)
    assert cases and int(cases.group(1)) > 100000, out[-2000:]
