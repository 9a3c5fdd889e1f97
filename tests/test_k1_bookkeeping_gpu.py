"""K1's sub-cube kernel (hk_sub.h) after its row entries carry finished store
slots (sub_rows.h) and its high-high distances are LDS broadcast reads: every
product configuration (13, 14, 15, 16 cities f64 and 16 cities i32), bit for
bit against the CPU oracle.

Per configuration a batch of 2 x CUs + 1 blocks, tiled from 24 distinct
matrices the oracle solves once per size:

  * 8 asymmetric non-integer matrices: a wrong store slot or a wrong distance
    address changes the cost bits;
  * 8 tie-heavy lattices (Euclidean, coordinates 0..3): the argmin must be the
    first strict minimum over the members ascending;
  * 8 asymmetric matrices of small integers (0..3): both at once.

(int32: the same matrices rounded to integers.)  The batch runs twice at the
product's occupancy, where it takes the sub-cube kernel with a block per
workgroup, and twice with one workgroup per CU (knob WG_PER_CU), where every
workgroup's persistent loop runs at least twice; each pair of runs must be
identical and every row equal to the oracle's cost bits and tour.  Nothing here
has a tolerance.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_py as O
import tspgpu

pytestmark = pytest.mark.gpu

F64, I32 = np.float64, np.int32
CASES = [(13, F64), (14, F64), (15, F64), (16, F64), (16, I32)]
DISTINCT = 24


def _euclid(xy):
    n = len(xy)
    return tspgpu.distance_matrix([[(i, xy[i, 0], xy[i, 1]) for i in range(n)]])[0]


def _matrices(n, dtype):
    rng = np.random.default_rng(7000 + n)
    out = []
    for b in range(DISTINCT):
        cls = b * 3 // DISTINCT
        if cls == 0:
            m = rng.uniform(0, 1000, (n, n))  # asymmetric, non-integer
        elif cls == 1:
            m = _euclid(rng.integers(0, 4, size=(n, 2)).astype(F64))  # tie-heavy lattice
        else:
            m = rng.integers(0, 4, size=(n, n)).astype(F64)  # asymmetric small integers
        np.fill_diagonal(m, 0.0)
        out.append(np.rint(m) if dtype == I32 else m)
    d = np.ascontiguousarray(np.array(out), dtype=dtype)
    assert len({m.tobytes() for m in d}) == DISTINCT
    return d


_REF = {}


def _reference(n, dtype):
    """(distinct matrices, oracle cost bits, oracle tours), solved once per case."""
    key = (n, np.dtype(dtype).name)
    if key not in _REF:
        d = _matrices(n, dtype)
        with ThreadPoolExecutor(max_workers=8) as ex:
            res = list(ex.map(lambda b: O.solve_block(np.asarray(d[b], dtype=F64)), range(DISTINCT)))
        cost = np.array([r[0] for r in res], dtype=F64)
        tours = np.array([r[1] for r in res], dtype=np.int32)
        if dtype == I32:
            assert np.array_equal(cost, np.rint(cost))
            bits = cost.astype(np.int64)
        else:
            bits = cost.view(np.uint64).copy()
        for a in (d, bits, tours):
            a.setflags(write=False)
        _REF[key] = (d, bits, tours)
    return _REF[key]


def _bits(cost):
    return cost.view(np.uint64) if cost.dtype == F64 else cost.astype(np.int64)


def _solve(ctx, d):
    return ctx.solve_blocks(d) if d.dtype == F64 else ctx.solve_blocks_i32(d)


def _run_twice_and_compare(ctx, batch, src, bits, tours):
    first = _solve(ctx, batch)
    assert ctx.last_variant() == 6
    second = _solve(ctx, batch)
    assert np.array_equal(_bits(first[0]), _bits(second[0])) and np.array_equal(first[1], second[1])
    T = tours.shape[1]
    bad = np.flatnonzero((_bits(first[0]) != bits[src]) | (first[1][:, :T] != tours[src]).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {batch.shape[0]} blocks differ from the oracle, first {bad[:5].tolist()}"


@pytest.mark.parametrize("n,dtype", CASES, ids=[f"n{n}-{np.dtype(t).name}" for n, t in CASES])
def test_sub_cube_kernel_matches_the_oracle_bit_for_bit(gpu_ctx, knobs, n, dtype):
    d, bits, tours = _reference(n, dtype)
    cu = gpu_ctx.device_info()[0]
    B = 2 * cu + 1
    src = np.random.default_rng(n).integers(0, DISTINCT, B)
    src[:DISTINCT] = np.arange(DISTINCT)  # (every distinct matrix is in the batch)
    batch = np.ascontiguousarray(d[src])
    # the product's occupancy: a block per workgroup
    _run_twice_and_compare(gpu_ctx, batch, src, bits, tours)
    assert gpu_ctx.last_grid() == B
    # one workgroup per CU: every workgroup solves two blocks, one of them three
    try:
        knobs.set("WG_PER_CU", 1)
        ctx = tspgpu.Context(device=0)
    finally:
        knobs.clear()
    try:
        _run_twice_and_compare(ctx, batch, src, bits, tours)
        assert ctx.last_grid() == cu and B > 2 * ctx.last_grid()
    finally:
        ctx.close()
