#!/usr/bin/env python3
"""Generate tests/golden/wide_large.json: instances past the sizes the suite
can solve on the CPU inside a test (n = 23 .. 26), each with the cost and tour
of the project's own CPU oracle (oracle/oracle.c through tests/oracle_py.py).

    python tests/golden/make_wide_golden.py [--out FILE] [n ...]

Needs nothing but oracle/liboracle.so.  The oracle's dense table is
N * 2^N doubles (3.2 GB at n = 25, 6.7 GB at n = 26) and a solve takes
5 s (n = 23) to 45 s (n = 26), so this runs once, not in a test.  Three
instances per n:

  uniform  n cities uniform in [0, 1000)^2
  lattice  n cities on integer coordinates in [0, 5)^2: coincident cities and
           many tied optima, so the tour is the tie rule's ("smallest m whose
           candidate equals the state value") at every layer
  integer  an asymmetric random int32 matrix, values 1..1000, zero diagonal,
           stored itself; the oracle solves it as doubles (every sum exact)

Every float is stored twice: exact C99 hex (the value compared) and %.17g
(for humans).  Seeded: two runs write byte-identical files.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_py as O  # noqa: E402

SEED = 20261020
KINDS = ("uniform", "lattice", "integer")


def instance(n: int, kind: str):
    """-> (json fields of the input, the (n, n) float64 matrix the oracle solves)"""
    rng = np.random.default_rng([SEED, n, KINDS.index(kind)])
    if kind == "integer":
        m = rng.integers(1, 1001, size=(n, n)).astype(np.int32)
        np.fill_diagonal(m, 0)
        return {"matrix": m.tolist()}, m.astype(np.float64)
    xy = rng.integers(0, 5, size=(n, 2)).astype(np.float64) if kind == "lattice" else rng.uniform(0, 1000, size=(n, 2))
    cities = [(i, float(xy[i, 0]), float(xy[i, 1])) for i in range(n)]
    return {"cities": [[c, x.hex(), y.hex()] for (c, x, y) in cities]}, O.distance_matrix(cities)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="*", type=int, default=[23, 24, 25, 26])
    ap.add_argument("--out", default=os.path.join(HERE, "wide_large.json"))
    args = ap.parse_args()
    data = []
    for n in sorted(args.n):
        for kind in KINDS:
            fields, d = instance(n, kind)
            cost, tour = O.solve_block(d)
            data.append({"n": n, "kind": kind, **fields, "cost_hex": float(cost).hex(), "cost": "%.17g" % cost,
                         "tour": tour})
            print(f"n={n} {kind}: cost {cost!r}", flush=True)
    out = {"generator": "tests/golden/make_wide_golden.py",
           "source": "oracle/oracle.c (oracle_solve_block), gcc -O2 -ffp-contract=off", "data": data}
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
