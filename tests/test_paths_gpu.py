"""Fixed-end shortest paths on the GPU (tspgpu_solve_paths*):
w cities, the first the fixed start and the last the fixed end, solved as K1
on the folded (w-1) x (w-1) matrix.

Nothing here has a tolerance: costs are compared bit for bit and orders entry
by entry with the CPU oracle on the folded matrix (tests/refine_model.py), and
for w <= 9 the cost also with a brute force over every interior permutation.
w = 11 is K1's 10 cities (the table in LDS), w = 12, 14, 17, 20 its 11, 13, 16
and 19."""
import errno
import math

import numpy as np
import pytest

import oracle_py as O
import refine_model as R
import tspgpu

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE


def city_blocks(w, B, kind, seed):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        if kind == "uniform":
            xy = rng.uniform(0, 1000, size=(w, 2))
        elif kind == "lattice":
            xy = rng.integers(0, 5, size=(w, 2)).astype(float)
        else:  # coincident: three sites only
            xy = rng.uniform(0, 1000, size=(3, 2))[rng.integers(0, 3, size=w)]
        out.append([(b * w + i, float(xy[i, 0]), float(xy[i, 1])) for i in range(w)])
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_against_oracle(dist, cost, order, status, brute=False):
    for b, D in enumerate(dist):
        oc, oo, ost = R.solve_path(D)
        assert status[b] == ost == 0, b
        assert same_bits(cost[b], oc), (b, cost[b], oc)
        assert order[b].tolist() == oo, b
        if brute:
            assert float(cost[b]) == R.brute_force(D), b


@pytest.mark.parametrize("kind", ["uniform", "coincident", "lattice"])
@pytest.mark.parametrize("w", [4, 5, 6, 8, 9])
def test_small_paths_against_brute_force_and_oracle(gpu_ctx, w, kind):
    blocks = city_blocks(w, 64, kind, 31 * w)
    cost, order, status = gpu_ctx.solve_paths_cities(blocks)
    dist = tspgpu.distance_matrix(blocks)
    check_against_oracle(dist, cost, order, status, brute=True)
    # the matrix form on the same matrices gives the same answers
    c2, o2, s2 = gpu_ctx.solve_paths(dist)
    assert same_bits(c2, cost) and np.array_equal(o2, order) and not s2.any()


@pytest.mark.parametrize("w", [11, 12, 14, 17, 20])
def test_larger_paths_against_oracle(gpu_ctx, w):
    blocks = city_blocks(w, 8, "uniform", w)
    cost, order, status = gpu_ctx.solve_paths_cities(blocks)
    check_against_oracle(tspgpu.distance_matrix(blocks), cost, order, status)


def test_w14_from_one_block_per_cu_runs_variant_6(gpu_ctx):
    cus, _ = gpu_ctx.device_info()
    blocks = city_blocks(14, cus + 3, "uniform", 14)
    cost, order, status = gpu_ctx.solve_paths_cities(blocks)
    assert gpu_ctx.last_variant() == 6
    check_against_oracle(tspgpu.distance_matrix(blocks), cost, order, status)


@pytest.mark.parametrize("w", [4, 7, 13])
def test_matrix_form_reads_neither_row_end_nor_column_start(gpu_ctx, w):
    rng = np.random.default_rng(w)
    D = rng.uniform(1, 100, size=(6, w, w))  # asymmetric
    clean = [R.solve_path(d) for d in D]
    D[:, w - 1, :] = math.nan
    D[:, :, 0] = -3.0
    cost, order, status = gpu_ctx.solve_paths(D)
    assert not status.any()
    for b in range(6):
        assert same_bits(cost[b], clean[b][0]) and order[b].tolist() == clean[b][1]
    Di = rng.integers(0, 1000, size=(6, w, w)).astype(np.int32)
    clean = [R.solve_path(d) for d in Di]
    Di[:, w - 1, :] = -5
    Di[:, :, 0] = -9
    cost, order, status = gpu_ctx.solve_paths(Di)
    assert cost.dtype == np.int32 and not status.any()
    for b in range(6):
        assert float(cost[b]) == clean[b][0] and order[b].tolist() == clean[b][1]


def test_device_pointer_forms(gpu_ctx):
    w, B = 9, 5
    blocks = city_blocks(w, B, "uniform", 99)
    arr, _, _ = tspgpu.cities_array(blocks)
    want = gpu_ctx.solve_paths_cities(blocks)
    d_c = gpu_ctx.upload(np.frombuffer(arr, np.uint8))
    d_d = gpu_ctx.upload(tspgpu.distance_matrix(blocks))
    d_cost, d_ord, d_st = gpu_ctx.upload(np.full(B, 7.0)), gpu_ctx.upload(np.full(B * w, 7, np.int32)), \
        gpu_ctx.upload(np.full(B, 7, np.int32))
    try:
        for run in (lambda: gpu_ctx.solve_paths_cities_device(d_c, w, B, d_cost, d_ord, d_st, gpu_ctx.stream),
                    lambda: gpu_ctx.solve_paths_device(d_d, tspgpu.F64, w, B, d_cost, d_ord, d_st, gpu_ctx.stream)):
            run()
            gpu_ctx.synchronize(gpu_ctx.stream)
            assert same_bits(gpu_ctx.download(d_cost, (B,), np.float64), want[0])
            assert np.array_equal(gpu_ctx.download(d_ord, (B, w), np.int32), want[1])
            assert not gpu_ctx.download(d_st, (B,), np.int32).any()
    finally:
        for p in (d_c, d_d, d_cost, d_ord, d_st):
            gpu_ctx.free(p)


def test_bad_blocks_cost_only_themselves(gpu_ctx):
    w = 8
    blocks = city_blocks(w, 6, "uniform", 8)
    cid, x, y = blocks[1][3]
    blocks[1][3] = (cid, math.nan, y)
    cid, x, y = blocks[4][0]
    blocks[4][0] = (cid, x + 1.0e9, y)
    cost, order, status = gpu_ctx.solve_paths_cities(blocks)
    assert status.tolist() == [0, EINVAL, 0, 0, ERANGE, 0]
    for b in (1, 4):
        assert math.isnan(cost[b]) and (order[b] == -1).all()
    good = [0, 2, 3, 5]
    dist = tspgpu.distance_matrix([blocks[b] for b in good])
    check_against_oracle(dist, cost[good], order[good], status[good], brute=True)
    # the same through the integer matrix form: -1 for the cost
    Di = np.random.default_rng(3).integers(0, 1000, size=(3, w, w)).astype(np.int32)
    Di[1, 2, 3] = -1
    ci, oi, si = gpu_ctx.solve_paths(Di)
    assert si.tolist() == [0, EINVAL, 0] and ci[1] == -1 and (oi[1] == -1).all()
    for b in (0, 2):
        oc, oo, _ = R.solve_path(Di[b])
        assert float(ci[b]) == oc and oi[b].tolist() == oo


def test_strict_context_refuses_w18():
    ctx = tspgpu.Context(device=0, strict=True)
    try:
        with pytest.raises(tspgpu.TspGpuError) as e:
            ctx.solve_paths_cities(city_blocks(18, 2, "uniform", 1))
        assert e.value.code == EINVAL
        blocks = city_blocks(17, 2, "uniform", 2)
        cost, order, status = ctx.solve_paths_cities(blocks)
        check_against_oracle(tspgpu.distance_matrix(blocks), cost, order, status)
    finally:
        ctx.close()
