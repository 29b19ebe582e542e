"""tf::LockedRanges (csrc/tf_locked_ranges.h), the process-wide registry of page-locked caller ranges behind
tf_host_register: sharing, containment, overlap and the last release, as a stand-alone program -- once plain, once under
AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(flags, out):
    src = os.path.join(ROOT, "tests", "cpp", "locked_ranges_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", out)
    subprocess.run(["g++", "-std=c++14", "-O1", "-g"] + flags + [src, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("flags,out", [([], "locked_ranges_test"),
                                       (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "locked_ranges_test_san")],
                         ids=["plain", "asan_ubsan"])
def test_locked_ranges(flags, out):
    r = subprocess.run([_build(flags, out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOCKED RANGES OK" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr[-2000:]
