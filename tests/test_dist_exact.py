"""The exactness rules of the device distance build on the CPU
(csrc/dist_exact.h): `make check-dist-exact` builds host/check_dist_exact.cpp
twice, plainly and under AddressSanitizer + UBSan, and runs both programs
directly.

The program includes the header as host code and checks against glibc's pow
and sqrt (called through volatile pointers, -fno-builtin-pow): a square the
rule does not flag has pow(dx, 2)'s bits, pow(-dx, 2) == pow(dx, 2),
sqrt_rn(a) has sqrt(a)'s bits and its acceptance test refuses both
neighbours.  Inputs: over 1e7 coordinate differences drawn like
tsphost_generate_grid's, integer and lattice differences, 0, values around
powers of two, tiny (< 2^-460) and huge (> 2^510) values; for sqrt_rn sums of
two such squares, perfect squares and powers of four.  It fails unless the
generator sample holds at least 1000 values with pow(dx, 2) != dx*dx (the
rule would otherwise go untested) and flags fewer than 12% of them (so that
flagging everything cannot pass; the rule alone gives 10.0%)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_rules_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-dist-exact"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    ok = re.findall(r"check_dist_exact: ok \((\d+) generator differences: (\d+) with pow != x\*x, ([0-9.]+)% flagged",
                    p.stdout)
    assert len(ok) == 2 and ok[0] == ok[1], p.stdout
    values, differ, share = int(ok[0][0]), int(ok[0][1]), float(ok[0][2])
    assert values >= 10_000_000 and differ >= 1000 and share < 12.0, ok[0]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
