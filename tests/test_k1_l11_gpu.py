"""K1 variant 6 with eleven low cities: configuration 65 of csrc/k1_cfg.h
(hk_sub_kernel<double, 15, 11, 512, 3>: 16 cities, 16 sub-cubes of 2048 rows,
512-thread workgroups, three per CU), forced through the knobs K1 = 6 and
TILED_CFG = 65 and compared bit for bit — costs by their bits, tours as
lists, no tolerance — with

  * the reference's own outputs for the 16-city batch of
    tests/golden/k1_batches.json (522 blocks; every third is a 0..3 lattice,
    every third a 0..39 lattice: the tie goldens there are at 16 cities —
    tests/golden/tie_blocks.json stops at 14, a size this configuration does
    not take);
  * the CPU oracle (tests/oracle_py) on a handful of generated blocks:
    lattices, uniform cities, asymmetric matrices, asymmetric small integers.

Batch sizes are the ones where a launch can go wrong: one block (a grid of
one workgroup), two, a few blocks cut into chunks of three and of two (a
later chunk's block uses slot blk - blk0 but cost and tour row blk), and the
smallest batch larger than the configuration's grid of three workgroups per
CU, where the forward kernel's persistent loop takes a second block.

Which configuration ran: with TILED_CFG set, k1_launch.cpp's pick_sub returns
that row or none (the dispatch then falls back to variant 4), so
last_variant() == 6 means configuration 65; the grid of the large batch
(three workgroups per CU, not configuration 60's six) says it once more.
"""
import numpy as np
import pytest

import oracle_py as O
import tspgpu
from test_k1_persistent_gpu import mixed_blocks

pytestmark = pytest.mark.gpu

CFG = 65
N = 16

_DATA = {}


def _golden():
    """(distance matrices, cost bits, tours as local indices) of the 16-city golden batch."""
    if "golden" not in _DATA:
        case = next(c for c in O.load_golden("k1_batches.json") if c["n"] == N)
        blocks = O.k1_batch_blocks(case)
        d = tspgpu.distance_matrix(blocks)
        cost = np.array([O.hexf(b["cost_hex"]) for b in case["blocks"]], dtype=np.float64)
        tours = np.array([[i - b["id0"] for i in b["ids"]] for b in case["blocks"]], dtype=np.int32)
        lattice = [i for i, b in enumerate(case["blocks"]) if isinstance(b["xy"][0][0], int)]
        assert tours.shape == (len(blocks), tspgpu.tour_length(N)) and len(lattice) >= len(blocks) // 2
        for a in (d, cost, tours):
            a.setflags(write=False)
        _DATA["golden"] = (d, cost.view(np.uint64), tours, lattice)
    return _DATA["golden"]


def _generated():
    """Ten generated blocks (two of each class of mixed_blocks) with the oracle's answers."""
    if "gen" not in _DATA:
        d = mixed_blocks(N, 10, 6511)
        res = [O.solve_block(m) for m in d]
        cost = np.array([r[0] for r in res], dtype=np.float64)
        tours = np.array([r[1] for r in res], dtype=np.int32)
        for a in (d, cost, tours):
            a.setflags(write=False)
        _DATA["gen"] = (d, cost.view(np.uint64), tours)
    return _DATA["gen"]


def _open(knobs, **more):
    try:
        for k, v in dict(K1=6, TILED_CFG=CFG, **more).items():
            knobs.set(k, v)
        return tspgpu.Context(device=0)
    finally:
        knobs.clear()


def _check(ctx, d, bits, tours):
    cost, tour = ctx.solve_blocks(np.ascontiguousarray(d))
    assert ctx.last_variant() == 6  # (with TILED_CFG = 65: that configuration, see the module's head)
    L = tours.shape[1]
    bad = np.flatnonzero((cost.view(np.uint64) != bits) | (tour[:, :L] != tours).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {len(bits)} blocks differ, first {bad[:5].tolist()}"
    assert (tour[:, L:] == -1).all()


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_blocks(knobs, B):
    d, bits, tours, lattice = _golden()
    gd, gbits, gtours = _generated()
    ctx = _open(knobs)
    try:
        # a tie-heavy lattice block first, then the batch's first blocks, then generated ones
        for start in (lattice[0], 0, 1, 2):
            _check(ctx, d[start:start + B], bits[start:start + B], tours[start:start + B])
            assert ctx.last_grid() == B
        for start in range(0, 10, 3):
            _check(ctx, gd[start:start + B], gbits[start:start + B], gtours[start:start + B])
    finally:
        ctx.close()


@pytest.mark.parametrize("chunk", [3, 2])
def test_a_few_blocks_in_several_chunks(knobs, chunk):
    gd, gbits, gtours = _generated()
    d, bits, tours, lattice = _golden()
    ctx = _open(knobs, K1_CHUNK=chunk)
    try:
        _check(ctx, gd[:7], gbits[:7], gtours[:7])  # chunks of 3, 3, 1 / 2, 2, 2, 1
        pick = lattice[:4] + [1, 2, 4]
        _check(ctx, d[pick], bits[pick], tours[pick])
    finally:
        ctx.close()


def test_golden_batch_and_the_persistent_loop(knobs):
    """The whole golden batch in one launch, then the smallest batch above the
    grid (3 x CUs + 5 blocks, rows of the golden batch again): five workgroups
    take a second block."""
    d, bits, tours, _ = _golden()
    ctx = _open(knobs)
    try:
        _check(ctx, d, bits, tours)
        cu = ctx.device_info()[0]
        src = np.arange(3 * cu + 5) % d.shape[0]
        _check(ctx, d[src], bits[src], tours[src])
        assert ctx.last_grid() == 3 * cu
    finally:
        ctx.close()


def test_one_workgroup_per_cu_and_a_second_chunk(knobs):
    """WG_PER_CU = 1 (a grid of one workgroup per CU) and chunks of 300: the
    first chunk's workgroups loop, the second chunk has the last 222 blocks."""
    d, bits, tours, _ = _golden()
    ctx = _open(knobs, WG_PER_CU=1, K1_CHUNK=300)
    try:
        _check(ctx, d, bits, tours)
        assert ctx.last_grid() == ctx.device_info()[0] < 300
    finally:
        ctx.close()


def test_same_bits_as_configuration_60(knobs):
    d, _, _, _ = _golden()
    gd, _, _ = _generated()
    both = np.ascontiguousarray(np.concatenate([d, gd]))
    out = {}
    for cfg in (60, CFG):
        try:
            knobs.set("K1", 6)
            knobs.set("TILED_CFG", cfg)
            ctx = tspgpu.Context(device=0)
        finally:
            knobs.clear()
        try:
            out[cfg] = ctx.solve_blocks(both)
            assert ctx.last_variant() == 6
        finally:
            ctx.close()
    assert np.array_equal(out[60][0].view(np.uint64), out[CFG][0].view(np.uint64))
    assert np.array_equal(out[60][1], out[CFG][1])
