"""The Or-opt stage's host plan on the CPU (csrc/or_opt_plan.h,
csrc/or_opt_plan.cpp): `make check-or-opt` builds host/check_or_opt.cpp with
the plan twice, plainly and under AddressSanitizer + UBSan, and runs both
programs directly.

The program counts its expectations on its own: the greedy selection against
a quadratic restatement on random candidate sets and on the adversarial ones
(all nested, chains sharing an edge, chains that only touch, equal gains, one
move reported by both of its ends, a forward and a backward move over one
range, one candidate, none), the range, rotation code and length prefix of
every accepted move, and every way a candidate can lie outside the contract.
Any sanitizer report aborts the second run (-fno-sanitize-recover=all)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_plan_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-or-opt"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    ok = re.findall(r"^check_or_opt: ok \((\d+) cases, (\d+) moves\)$", p.stdout, flags=re.M)
    assert len(ok) == 2 and ok[0] == ok[1], p.stdout
    assert int(ok[0][0]) > 1200 and int(ok[0][1]) > 5000, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
