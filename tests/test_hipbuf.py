"""The owner type of every HIP handle on the CPU (csrc/hipbuf.h): `make
check-hipbuf` builds host/check_hipbuf.cpp twice, plainly and under
AddressSanitizer + UBSan, and runs both programs directly.

The program instantiates Owned with a counting fake free function, so no HIP
call is made, and checks move construction, move assignment, self-move
assignment, reset twice, a vector of owners growing, that a moved-from or
default owner frees nothing and that every handle is freed exactly once; and
the one HIP-error-to-errno mapping.  Any sanitizer report aborts the second run
(-fno-sanitize-recover=all)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_owner_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-hipbuf"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert len(re.findall(r"^check_hipbuf: ok$", p.stdout, flags=re.M)) == 2 and "FAIL" not in p.stdout, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
