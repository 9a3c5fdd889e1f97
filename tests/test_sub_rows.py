"""K1 variant 6's row table on the CPU (csrc/sub_rows.h, csrc/sub_rows.cpp):
`make check-sub-rows` builds host/check_sub_rows.cpp with the builder twice,
plainly and under AddressSanitizer + UBSan, and runs both programs directly.

The program checks, for every L the builder accepts (5..10), every J in
2..L-2, every mask of J bits and every non-member k_q: the nibbles list the
members then the non-members ascending; the q-th slot field decodes to
(k_q - q) * C(L, J+1) + the colex rank of mask | (1 << k_q) and is below
C(L, J+1) * (J+1); no two fields overlap; no field crosses a 32-bit word;
every unused bit is zero.  It computes binomials and ranks on its own (Pascal's
triangle), not with the header's functions.  Any sanitizer report aborts the
second run (-fno-sanitize-recover=all)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_row_table_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-sub-rows"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    # one line per program; the field count is sum over L, J of C(L, J) * (L - J)
    want = sum(_binom(L, J) * (L - J) for L in range(5, 11) for J in range(2, L - 1))
    assert p.stdout.count(f"check_sub_rows: ok (L = 5..10, {want} slot fields)") == 2, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def _binom(a, b):
    r = 1
    for i in range(1, b + 1):
        r = r * (a - b + i) // i
    return r
