"""The ragged batch plan on the CPU (csrc/ragged_plan.h, csrc/ragged_plan.cpp):
`make check-ragged` builds host/check_ragged.cpp with the planner twice, plainly
and under AddressSanitizer + UBSan, and runs both programs directly.

The program computes its expectations on its own (std::stable_sort of the
block indices by n, running sums for the bucket positions) and checks, for
both value sizes, strict and not: empty and one-block batches, one size, every
size 2..20, 1000 random sizes, a size with no block between two that have some,
n of -3, 0, 1, 21 and 17, negative offsets, repeated, descending, overlapping
and odd-gap offsets.  Per case: refused blocks carry -EINVAL and are in no
bucket; slots are a bijection onto the bucket positions in caller order;
bucket bases are 256-byte aligned and no two buckets or blocks overlap; the
covering extent and the largest n.  Any sanitizer report aborts the second run
(-fno-sanitize-recover=all)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_plan_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-ragged"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    ok = re.findall(r"^check_ragged: ok \((\d+) cases, (\d+) blocks\)$", p.stdout, flags=re.M)
    assert len(ok) == 2 and ok[0] == ok[1], p.stdout
    # 15 cases for each of (f64, i32) x (strict, not)
    assert int(ok[0][0]) == 60 and int(ok[0][1]) > 8000, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
