"""The scan's tile split and its LEAP2 LDS reservation, exhaustively on the host (tools/tile_split_check.cpp).

filter_groupby_kernel buffers one STATS_LEAP2 byte per (tile, wave) of a workgroup's run in LDS and its tile loop has
no bound: the plan must reserve the longest run any workgroup of any of its launches can take, slot weights included
(pgpu_config.slot_weight_step).  The split and the reservation are one header (pinot_amd/csrc/tile_split.h) shared by
the kernel, the plan and this check, which is compiled alone under AddressSanitizer + UndefinedBehaviorSanitizer
(pinot_amd.build.build_tile_split_check) and run as a program: grids 1..80 and the multiples of 8 around 256 CUs x
1..8, T up to 40 x grid plus 36 900 and 123 000, 2-4 slots per CU, steps 0 / 0.11 / 1 / 3 / 4, launches smaller than
their plan, T up to INT32_MAX on up to 65 536 workgroups.  It asserts that every tile is scanned exactly once, that no
run passes the reservation or the cap, and that weighted runs are their shares.  No GPU is touched.
"""
import os
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
    return build.build_tile_split_check()


def _run(check, *args):
    res = subprocess.run([check, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=ENV,
                         timeout=300)
    return res.returncode, res.stdout


def test_tile_split_partitions_and_fits_the_reservation(check):
    rc, out = _run(check)
    assert rc == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert " 0 failures" in out, out[-2000:]


def test_check_rejects_the_equal_share_reservation(check):
    """The check has teeth: against ceil(tiles / grid) + 3, the reservation before the weights were accounted for, it
    fails -- among others at the default step on 300 segments of 123 tiles (36 900 tiles, 1 024 workgroups, 4 per CU,
    step 0.11: a 42-tile run on 40 reserved)."""
    rc, out = _run(check, "--parent-reservation")
    assert rc == 1, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert ("FAIL longest run exceeds the LEAP2 reservation: 42 vs 40  (plan B=36900 G=1024 slots=4 step=0.11; "
            "launch T=36900 grid=1024 chunks=1)") in out.splitlines(), out[:6000]
