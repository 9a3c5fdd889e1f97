"""K1 variant 6's row table at L = 11 on the CPU (csrc/sub_rows.h,
csrc/sub_rows.cpp; configuration 65 of csrc/k1_cfg.h decodes it).

Eleven nibbles leave 84 bits for the slot fields, so L = 11 is the first size
where the header picks other layouts than "whole slot, no field crosses a
32-bit word": fields packed back to back at J = 2, 4, 5 (a field may straddle
two words) and rank-only fields at J = 3 (the decoder adds the layer offset of
the destination's position from its nibble).

  * `make check-sub-rows` (host/check_sub_rows.cpp, plain and under ASan +
    UBSan, both run directly) now also checks every J, mask and destination of
    L = 11 and prints a second line for it; the L = 5..10 line, with the
    original layout rule written out in the program, is
    tests/test_sub_rows.py's.
  * `check_sub_rows --dump 11` prints the header's layout (per J: rank-only
    flag, field width, field positions) and the built table.  This file
    decodes every entry with those numbers alone, the way hk_sub.h's sub_nib
    and sub_slot do (two-word extract where a field straddles), and compares
    members, non-members and finished slots with a recomputation from the mask
    by itertools and math.comb.
"""
import itertools
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")
L = 11

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


def test_row_table_l11_plain_and_sanitized():
    p = subprocess.run(["make", "-s", "-C", PKG, "check-sub-rows"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    want = sum(math.comb(L, J) * (L - J) for J in range(2, L - 1))
    assert p.stdout.count(f"check_sub_rows: ok (L = 11, {want} slot fields)") == 2, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def _bits(words, pos, width):
    """bits pos..pos+width-1 of the entry, from one word or from two"""
    v = words[pos // 32] >> (pos % 32)
    if pos % 32 + width > 32:
        v |= words[pos // 32 + 1] << (32 - pos % 32)
    return v & ((1 << width) - 1)


def test_every_l11_entry_decodes_to_its_definition():
    p = subprocess.run(["make", "-s", "-C", PKG, "bin/check_sub_rows"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    p = subprocess.run([os.path.join(PKG, "bin", "check_sub_rows"), "--dump", str(L)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    layout, entries, bit0 = {}, [], None
    for ln in p.stdout.splitlines():
        t = ln.split()
        if t[0] == "field_bit0":
            bit0 = int(t[1])
        elif t[0] == "layout":
            layout[int(t[1])] = (t[2] == "1", int(t[3]), [int(x) for x in t[4:]])
        elif t[0] == "entry":
            entries.append([int(x, 16) for x in t[1:]])
    assert bit0 == 4 * L and sorted(layout) == list(range(2, L - 1)) and len(entries) == 1 << L
    # the layouts the header documents: J = 3 rank only; J = 2, 4, 5 with a straddling field; J >= 6 without
    straddles = {J: any(pos // 32 != (pos + w - 1) // 32 for pos in ps) for J, (_, w, ps) in layout.items()}
    assert {J for J, (ro, _, _) in layout.items() if ro} == {3}
    assert {J for J, s in straddles.items() if s} == {2, 4, 5}
    # table order: by member count, then by value (= colex order of equal-size subsets)
    idx = 0
    checked = 0
    for J in range(L + 1):
        subsets = sorted(itertools.combinations(range(L), J), key=lambda s: sum(1 << b for b in s))
        rank = {s: r for r, s in enumerate(subsets)}
        nxt = sorted(itertools.combinations(range(L), J + 1), key=lambda s: sum(1 << b for b in s))
        nrank = {s: r for r, s in enumerate(nxt)}
        for mem in subsets:
            w = entries[idx]
            idx += 1
            non = [b for b in range(L) if b not in mem]
            nibs = [_bits(w, 4 * i, 4) for i in range(L)]
            assert nibs == list(mem) + non, (mem, nibs)
            used = (1 << (4 * L)) - 1
            if 2 <= J <= L - 2:
                rank_only, width, poss = layout[J]
                assert len(poss) == len(non) and min(poss) >= bit0 and max(poss) + width <= 128
                for q, k in enumerate(non):
                    dest = tuple(sorted(mem + (k,)))
                    want = (k - q) * math.comb(L, J + 1) + nrank[dest]  # position of k in dest = k - q
                    assert dest.index(k) == k - q
                    got = _bits(w, poss[q], width)
                    if rank_only:
                        got += (nibs[J + q] - q) * math.comb(L, J + 1)
                    assert got == want and got < math.comb(L, J + 1) * (J + 1), (mem, k, got, want)
                    field = ((1 << width) - 1) << poss[q]
                    assert not used & field
                    used |= field
                    checked += 1
            whole = w[0] | w[1] << 32 | w[2] << 64 | w[3] << 96
            assert not whole & ~used, (mem, hex(whole))
            assert rank[mem] == idx - 1 - sum(math.comb(L, i) for i in range(J))
    assert idx == 1 << L and checked == sum(math.comb(L, J) * (L - J) for J in range(2, L - 1))
