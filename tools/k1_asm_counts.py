#!/usr/bin/env python3
"""Static counts of one kernel of one K1 unit (CPU side, no GPU).

    python tools/k1_asm_counts.py hks_p60 [--kernel hk_sub_kernel] [--asm FILE]

Compiles tsp-mpi-reduction_amd/csrc/k1/UNIT.hip to gfx950 assembly with the
Makefile's flags (`make asm-unit`: --cuda-device-only -S) and prints, for the
one kernel whose symbol contains --kernel: code bytes, .vgpr_count,
.vgpr_spill_count, .sgpr_spill_count, LDS bytes, and the number of lines whose
mnemonic starts with v_, ds_ and buffer_.  Nothing else in the assembly is
looked at.  --asm FILE counts an assembly file made earlier (e.g. of another
commit's sources) instead of compiling.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tsp-mpi-reduction_amd")


def counts(text, kernel):
    lines = text.splitlines()
    # the kernel's body: from its label to the end-of-function label
    start = next((i for i, ln in enumerate(lines) if re.match(r"^\w+:", ln) and kernel in ln.split(":")[0]), None)
    if start is None:
        sys.exit(f"no kernel matching {kernel!r}")
    symbol = lines[start].split(":")[0]
    out = {"kernel": symbol, "v_": 0, "ds_": 0, "buffer_": 0}
    body = True
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            body = False
        m = re.match(r"^\s+([a-z_0-9]+)\b", ln) if body else None
        if m:
            for pre in ("v_", "ds_", "buffer_"):
                if m.group(1).startswith(pre):
                    out[pre] += 1
        # (the compiler's kernel-info comment follows the end-of-function label)
        m = re.match(r"^; codeLenInByte = (\d+)", ln)
        if m:
            out["code_bytes"] = int(m.group(1))
            break
    # the kernel's entry of the code object metadata (amdhsa.kernels)
    entry, cur = None, []
    for ln in lines:
        if ln.startswith("  - ."):
            cur = []
        cur.append(ln)
        if re.match(r"^\s+\.name:\s+" + re.escape(symbol) + r"\s*$", ln):
            entry = cur
    if entry is None:
        sys.exit(f"no metadata entry for {symbol}")
    for key, name in ((".vgpr_count", "vgpr_count"), (".vgpr_spill_count", "vgpr_spill_count"),
                      (".sgpr_spill_count", "sgpr_spill_count"), (".group_segment_fixed_size", "lds_bytes")):
        for ln in entry:
            m = re.match(r"^\s+(?:- )?" + re.escape(key) + r":\s+(\d+)", ln)
            if m:
                out[name] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("unit", help="a file of csrc/k1 without .hip, e.g. hks_p60")
    ap.add_argument("--kernel", default="hk_sub_kernel", help="substring of the kernel's symbol")
    ap.add_argument("--asm", default=None, help="count this assembly file instead of compiling")
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, args.unit + ".s")
            subprocess.run(["make", "-s", "-C", PKG, "asm-unit", f"UNIT=k1/{args.unit}", f"OUT={out}"], check=True)
            text = open(out).read()
    print(json.dumps(dict(unit=args.unit, **counts(text, args.kernel))))


if __name__ == "__main__":
    main()
