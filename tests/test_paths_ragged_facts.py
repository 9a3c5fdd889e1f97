"""The facts and rules of the ragged K1 -> K3 hand-off on the CPU
(csrc/paths_facts.h's total-count forms, csrc/block_desc.h):
`make check-paths-ragged` builds host/check_paths_ragged.cpp twice, plainly
and under AddressSanitizer + UBSan, and runs both programs directly.

The program runs a serial twin of the ragged summary and bitmap (packed
cities, tour rows of one stride, concatenated paths of different lengths)
against the scans the host front of tspgpu_reduce_ragged does, over random
ragged batches: every id layout of tests/test_paths_facts.py (the widest range
that fits, ending in a partial 32-bit word of the bitmap, included), 2-city
blocks mixed in, statuses, bad indices (one that a longer neighbour would
accept included) and non-finite coordinates."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


def test_ragged_rules_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-paths-ragged"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    ok = re.findall(r"check_paths_ragged: ok \((\d+) cases: (\d+) fold_ok, (\d+) wide id ranges, (\d+) duplicates, "
                    r"(\d+) open paths, (\d+) id ranges ending on the bitmap's last bit, (\d+) of them in a partial "
                    r"word, (\d+) with 2-city blocks, (\d+) with mixed sizes", p.stdout)
    assert len(ok) == 2 and ok[0] == ok[1], p.stdout
    v = [int(x) for x in ok[0]]
    assert v[0] >= 4000 and all(x >= 200 for x in v[1:6]) and v[6] >= 100 and v[7] >= 200 and v[8] >= 3000, v
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
