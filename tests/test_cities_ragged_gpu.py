"""Distances and K1 from PACKED ragged city blocks
(tspgpu_distance_matrix_ragged_device, tspgpu_solve_cities_ragged[_device];
DESIGN.md §6c).

Nothing here has a tolerance: every block's matrix is compared as uint64 bits
with tspgpu_distance_matrix on that block alone, costs bit for bit and tours
entry by entry with the CPU oracle on that matrix.  Cities are the reference
generator's (tests/test_cities_device_gpu.py's generator, whose squares the
exactness rule flags about one in ten of) unless a case says otherwise."""
import errno

import numpy as np
import pytest

import oracle_py as O
import tspgpu
from test_cities_device_gpu import _carray, _generated, _same_bits

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
U64 = np.uint64
# four different sizes share the first workgroup, the pair loop has 1, 2 and 3
# passes (1, 66 and 190 pairs), and the block count is no multiple of 4
MIXED = [2, 12, 20, 3, 20, 7, 16]


def ragged_cities(ns, seed=0):
    """Block b: the generator's block b (+ seed) of a batch of n[b]-city blocks -> list of (n_b,) CITY_DTYPE."""
    cache = {}
    out = []
    for b, n in enumerate(ns):
        if n not in cache:
            cache[n] = _generated(n, len(ns) + seed)
        out.append(cache[n][b + seed].copy())
    return out


def packed(blocks):
    return np.concatenate(blocks) if blocks else np.zeros(0, tspgpu.CITY_DTYPE)


def host_dist(blk):
    return tspgpu.distance_matrix_array(_carray(blk), len(blk), 1)[0]


def device_dist(ctx, blocks, stream=None):
    """distance_matrix_ragged_device on the uploaded packed cities -> list of (n_b, n_b) float64."""
    ns = [len(b) for b in blocks]
    st = ctx.stream if stream is None else stream
    d_c = ctx.upload(packed(blocks).view(np.uint8))
    elems = sum(n * n for n in ns)
    d_d = ctx.upload(np.full(elems, -7.0))
    try:
        ctx.distance_matrix_ragged_device(d_c, ns, d_d, st)
        ctx.synchronize(st)
        flat = ctx.download(d_d, (elems,), np.float64)
    finally:
        ctx.free(d_c)
        ctx.free(d_d)
    out, at = [], 0
    for n in ns:
        out.append(flat[at:at + n * n].reshape(n, n))
        at += n * n
    return out


def solve_device(ctx, blocks, stride=None, stream=None):
    """solve_cities_ragged_device on the uploaded packed cities -> (cost, tours (B, stride), status)."""
    ns = [len(b) for b in blocks]
    B = len(ns)
    stride = max(ns) + 1 if stride is None else stride
    st = ctx.stream if stream is None else stream
    d_c = ctx.upload(packed(blocks).view(np.uint8))
    d_cost, d_tour, d_st = ctx.upload(np.full(B, 7.0)), ctx.upload(np.full(B * stride, 7, np.int32)), \
        ctx.upload(np.full(B, 7, np.int32))
    try:
        ctx.solve_cities_ragged_device(d_c, ns, d_cost, d_tour, stride, d_st, st)
        ctx.synchronize(st)
        return (ctx.download(d_cost, (B,), np.float64), ctx.download(d_tour, (B, stride), np.int32),
                ctx.download(d_st, (B,), np.int32))
    finally:
        for p in (d_c, d_cost, d_tour, d_st):
            ctx.free(p)


def assert_oracle(blk, cost, row):
    """status 0: the cost bits and tour of the oracle on the block's host matrix, the row padded with -1"""
    oc, ot = O.solve_block(host_dist(blk))
    assert float(cost).hex() == oc.hex()
    L = tspgpu.tour_length(len(blk))
    assert row[:L].tolist() == ot and (row[L:] == -1).all(), row.tolist()


# ---- distances ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [MIXED, [20], [1, 5, 1]], ids=lambda v: "-".join(map(str, v)))
def test_matrix_bits_equal_the_host_build_of_each_block(gpu_ctx, ns):
    blocks = ragged_cities(ns)
    got = device_dist(gpu_ctx, blocks)
    sq, flagged, passes = gpu_ctx.cities_last_fixups()
    for b, blk in enumerate(blocks):
        assert _same_bits(got[b], host_dist(blk)), (b, len(blk))
    assert sq == sum(n * (n - 1) for n in ns) and flagged <= sq and passes == 1
    if ns == MIXED:
        assert flagged > 0  # (the comparison sees the fix-ups work)


def test_fixup_list_overflow_rebuilds_with_a_larger_list(gpu_ctx, knobs):
    blocks = ragged_cities(MIXED)
    knobs.set("DIST_FIX_CAP", 1)
    got = device_dist(gpu_ctx, blocks)
    sq, flagged, passes = gpu_ctx.cities_last_fixups()
    assert passes == 2 and flagged > 1
    for b, blk in enumerate(blocks):
        assert _same_bits(got[b], host_dist(blk)), (b, len(blk))


def test_uniform_batch_gives_the_uniform_forms_bytes(gpu_ctx):
    """n = [6]*5: the same device bytes (cost, tour rows of n + 1, status) as tspgpu_solve_cities_device."""
    n, B = 6, 5
    cs = _generated(n, B)
    cost, tour, status = solve_device(gpu_ctx, [cs[b] for b in range(B)])
    d_c = gpu_ctx.upload(np.ascontiguousarray(cs).view(np.uint8))
    d_cost, d_tour, d_st = gpu_ctx.upload(np.full(B, 7.0)), gpu_ctx.upload(np.full(B * (n + 1), 7, np.int32)), \
        gpu_ctx.upload(np.full(B, 7, np.int32))
    try:
        gpu_ctx.solve_cities_device(d_c, n, B, d_cost, d_tour, d_st, gpu_ctx.stream)
        gpu_ctx.synchronize()
        assert cost.tobytes() == gpu_ctx.download(d_cost, (B,), np.float64).tobytes()
        assert tour.tobytes() == gpu_ctx.download(d_tour, (B, n + 1), np.int32).tobytes()
        assert status.tobytes() == gpu_ctx.download(d_st, (B,), np.int32).tobytes()
    finally:
        for p in (d_c, d_cost, d_tour, d_st):
            gpu_ctx.free(p)


# ---- the solve forms ---------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [0, 3])
def test_solve_forms_equal_the_oracle(gpu_ctx, extra):
    """Device and host forms, tour_stride = max n + 1 and max n + 3."""
    blocks = ragged_cities(MIXED, seed=1)
    stride = max(MIXED) + 1 + extra
    cost, tour, status = solve_device(gpu_ctx, blocks, stride)
    assert not status.any(), status.tolist()
    for b, blk in enumerate(blocks):
        assert_oracle(blk, cost[b], tour[b])
    arr = _carray(packed(blocks))
    hcost, htour, hstatus = gpu_ctx.solve_cities_ragged((arr, [len(b) for b in blocks]), tour_stride=stride)
    assert hcost.tobytes() == cost.tobytes() and np.array_equal(htour, tour) and not hstatus.any()


def test_a_single_block_of_twenty(gpu_ctx):
    blocks = ragged_cities([20], seed=2)
    cost, tour, status = solve_device(gpu_ctx, blocks)
    assert status.tolist() == [0]
    want_cost, want_tour = gpu_ctx.solve_blocks(host_dist(blocks[0])[None])
    assert cost.tobytes() == want_cost.tobytes() and np.array_equal(tour, want_tour)


def test_non_finite_coordinates_cost_only_their_block(gpu_ctx):
    blocks = ragged_cities(MIXED, seed=3)
    blocks[1]["x"][5] = np.nan   # a NaN coordinate
    blocks[4]["y"][0] = 1e200    # 1e200 apart: the square overflows, an infinite distance
    got = device_dist(gpu_ctx, blocks)
    for b, blk in enumerate(blocks):
        want = host_dist(blk)
        if b in (1, 4):  # as the host gives them, a NaN's payload aside
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got[b]), nan)
            assert np.array_equal(got[b].view(U64)[~nan], want.view(U64)[~nan])
            assert tspgpu.validate(want[None]) == EINVAL
        else:
            assert _same_bits(got[b], want)
    cost, tour, status = solve_device(gpu_ctx, blocks)
    assert status.tolist() == [0, EINVAL, 0, 0, EINVAL, 0, 0]
    for b, blk in enumerate(blocks):
        if status[b]:
            assert np.isnan(cost[b]) and (tour[b] == -1).all()
        else:  # the neighbours: the bits of solve_blocks
            want_cost, want_tour = gpu_ctx.solve_blocks(host_dist(blk)[None])
            L = tspgpu.tour_length(len(blk))
            assert cost[b:b + 1].tobytes() == want_cost.tobytes()
            # (solve_blocks gives rows of n + 1 entries: a 2-city tour is [1, 0, -1])
            assert np.array_equal(tour[b, :L], want_tour[0, :L]) and (want_tour[0, L:] == -1).all()
            assert (tour[b, L:] == -1).all()
    hcost, htour, hstatus = gpu_ctx.solve_cities_ragged((_carray(packed(blocks)), MIXED))  # returns 0
    assert hstatus.tolist() == status.tolist() and np.array_equal(htour, tour)
    assert np.array_equal(hcost.view(U64)[status == 0], cost.view(U64)[status == 0])


def test_strict_context_refuses_an_extension_size_per_block():
    ctx = tspgpu.Context(device=0, strict=True)
    try:
        blocks = ragged_cities([5, 18, 5], seed=4)
        cost, tour, status = solve_device(ctx, blocks)
        assert status.tolist() == [0, EINVAL, 0]
        assert np.isnan(cost[1]) and (tour[1] == -1).all()
        for b in (0, 2):
            assert_oracle(blocks[b], cost[b], tour[b])
    finally:
        ctx.close()


def test_argument_errors_with_a_context(gpu_ctx):
    blocks = ragged_cities([5, 7, 5])
    for bad in ([5, 0, 5], [5, 21, 5], [5, -3, 5]):
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.solve_cities_ragged((_carray(packed(blocks)), bad), tour_stride=22)
        assert e.value.code == EINVAL
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_cities_ragged((_carray(packed(blocks)), [5, 7, 5]), tour_stride=7)
    assert e.value.code == EINVAL
    cost, tour, status = gpu_ctx.solve_cities_ragged((_carray(packed(blocks)), [5, 7, 5]))
    assert not status.any()
