"""Distances on the device (tspgpu_distance_matrix_device,
tspgpu_solve_cities_device, tspgpu_solve_cities_upload).

Nothing here has a tolerance: matrices and costs are compared as uint64 bits
against the host path (tspgpu_distance_matrix with glibc's pow and sqrt,
Context.solve_cities), tours entry by entry.  Cities are the reference
generator's (`./tsp n B 1000 1000`, bench.Shard) unless a case says otherwise."""
import ctypes
import errno
import math
import os
import re
import subprocess

import numpy as np
import pytest

import tspgpu
from bench import Shard

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE
U64 = np.uint64


def _generated(n, B):
    """(B, n) CITY_DTYPE array of the generator's cities."""
    s = Shard(n, B, 0, B)
    return np.frombuffer(s.arr, dtype=tspgpu.CITY_DTYPE).reshape(B, n).copy()


def _carray(cs):
    cs = np.ascontiguousarray(cs)
    return (tspgpu.City * cs.size).from_buffer_copy(cs.tobytes())


def _host_dist(cs):
    B, n = cs.shape
    return tspgpu.distance_matrix_array(_carray(cs), n, B)


def _device_dist(ctx, cs, stream=None):
    """distance_matrix_device on uploaded cities -> (B, n, n) float64."""
    B, n = cs.shape
    st = ctx.stream if stream is None else stream
    d_c = ctx.upload(np.ascontiguousarray(cs).view(np.uint8))
    d_d = ctx.upload(np.full(B * n * n, -7.0))
    try:
        ctx.distance_matrix_device(d_c, n, B, d_d, st)
        ctx.synchronize(st)
        return ctx.download(d_d, (B, n, n), np.float64)
    finally:
        ctx.free(d_c)
        ctx.free(d_d)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(U64), b.view(U64))


def _solve_device(ctx, cs, stream=None):
    """solve_cities_device on uploaded cities -> (cost, tours (B, n+1), status)."""
    B, n = cs.shape
    st = ctx.stream if stream is None else stream
    d_c = ctx.upload(np.ascontiguousarray(cs).view(np.uint8))
    d_cost, d_tour, d_st = ctx.upload(np.full(B, 7.0)), ctx.upload(np.full(B * (n + 1), 7, np.int32)), \
        ctx.upload(np.full(B, 7, np.int32))
    try:
        ctx.solve_cities_device(d_c, n, B, d_cost, d_tour, d_st, st)
        ctx.synchronize(st)
        return (ctx.download(d_cost, (B,), np.float64), ctx.download(d_tour, (B, n + 1), np.int32),
                ctx.download(d_st, (B,), np.int32))
    finally:
        for p in (d_c, d_cost, d_tour, d_st):
            ctx.free(p)


# 1 -----------------------------------------------------------------------------------------------

def test_matrix_parity_large_batch_with_real_pow_mismatches(gpu_ctx):
    """4096 blocks of 16 cities: ~1 M squares, of which ~800 have
    pow(dx, 2) != dx*dx (counted here with the C library's pow: at least 100,
    or the comparison would not see the fix-ups work)."""
    cs = _generated(16, 4096)
    i, j = np.triu_indices(16, 1)
    diffs = np.concatenate([(cs["x"][:, i] - cs["x"][:, j]).ravel(), (cs["y"][:, i] - cs["y"][:, j]).ravel()])
    squares = diffs * diffs
    differ = sum(1 for v, p in zip(diffs.tolist(), squares.tolist()) if math.pow(v, 2) != p)
    print(f"pow(dx,2) != dx*dx for {differ} of {diffs.size} squares")
    assert differ >= 100
    got = _device_dist(gpu_ctx, cs)
    sq, flagged, passes = gpu_ctx.cities_last_fixups()
    print(f"squares {sq} flagged {flagged} ({100.0 * flagged / sq:.2f}%) build passes {passes}")
    assert _same_bits(got, _host_dist(cs))
    assert sq == diffs.size == 4096 * 16 * 15
    assert 0 < flagged < 0.12 * sq and passes == 1


@pytest.mark.parametrize("n", range(1, 21))
def test_matrix_parity_every_size(gpu_ctx, n):
    """3 blocks of every n: n = 1 has no pair, n = 2 one, n = 12 has 66 (just
    past one wave's 64 lanes), n = 20 has 190 (three passes)."""
    cs = _generated(n, 3)
    assert _same_bits(_device_dist(gpu_ctx, cs), _host_dist(cs))
    sq, flagged, passes = gpu_ctx.cities_last_fixups()
    assert sq == 3 * n * (n - 1) and flagged <= sq and passes == 1


def test_matrix_parity_coincident_and_lattice_blocks(gpu_ctx):
    cs = _generated(9, 3)
    cs["x"][0], cs["y"][0] = 123.456, 654.321  # every city of block 0 at one point
    rng = np.random.default_rng(4401)
    cs["x"][1] = rng.integers(0, 4, 9)  # block 1 on the lattice 0..3
    cs["y"][1] = rng.integers(0, 4, 9)
    got, want = _device_dist(gpu_ctx, cs), _host_dist(cs)
    assert _same_bits(got, want)
    assert not got[0].view(U64).any()  # +0.0 everywhere, never -0.0


# 2 -----------------------------------------------------------------------------------------------

def test_fixup_list_overflow_rebuilds_with_a_larger_list(gpu_ctx, knobs):
    cs = _generated(16, 256)
    knobs.set("DIST_FIX_CAP", 64)
    got = _device_dist(gpu_ctx, cs)
    sq, flagged, passes = gpu_ctx.cities_last_fixups()
    assert _same_bits(got, _host_dist(cs))
    assert passes == 2 and flagged > 64 and sq == 256 * 16 * 15


# 3 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(2, 21))
def test_solve_cities_device_equals_the_host_path(gpu_ctx, n):
    """522 blocks for 13..16 cities (a full wave of blocks: K1 variant 6), 64
    blocks for the other sizes."""
    B = 522 if 13 <= n <= 16 else 64
    cs = _generated(n, B)
    want_cost, want_tour = gpu_ctx.solve_cities((_carray(cs), n, B))
    cost, tour, status = _solve_device(gpu_ctx, cs)
    variant = gpu_ctx.last_variant()
    assert not status.any(), status.tolist()
    assert _same_bits(cost, want_cost)
    assert np.array_equal(tour, want_tour)
    if 13 <= n <= 16:
        assert variant == 6
    # the upload form, the same answers once more
    cost_u, tour_u = gpu_ctx.solve_cities((_carray(cs), n, B), device_dist=True)
    assert _same_bits(cost_u, want_cost) and np.array_equal(tour_u, want_tour)


# 4 -----------------------------------------------------------------------------------------------

def test_bad_blocks_cost_only_themselves(gpu_ctx):
    n, B = 16, 12
    cs = _generated(n, B)
    cs["x"][2, 5] = np.nan    # a NaN coordinate
    cs["y"][6, 0] = 1e200     # 1e200 apart: the square overflows, an infinite distance
    cs["x"][9, 15] += 2e8     # 2e8 apart: n * max d >= INT_MAX
    host = _host_dist(cs)
    want_status = [tspgpu.validate(host[b:b + 1]) for b in range(B)]
    assert [want_status[b] for b in (2, 6, 9)] == [EINVAL, EINVAL, ERANGE]
    good = [b for b in range(B) if not want_status[b]]
    assert len(good) == B - 3
    want_cost, want_tour = gpu_ctx.solve_cities((_carray(cs[good]), n, len(good)))
    cost, tour, status = _solve_device(gpu_ctx, cs)
    assert status.tolist() == want_status
    for b in (2, 6, 9):
        assert np.isnan(cost[b]) and (tour[b] == -1).all(), (b, cost[b], tour[b].tolist())
    assert _same_bits(cost[good], want_cost) and np.array_equal(tour[good], want_tour)
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_cities((_carray(cs), n, B), device_dist=True)
    assert e.value.code == EINVAL  # the first bad block's code, as the host path gives
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_cities((_carray(cs), n, B))
    assert e.value.code == EINVAL
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_cities((_carray(cs[9:]), n, B - 9), device_dist=True)
    assert e.value.code == ERANGE


def test_argument_errors_with_a_context(gpu_ctx):
    """Decided before any device work: nothing is launched, nothing written."""
    L, h = tspgpu.lib(), gpu_ctx.handle
    cs = _generated(5, 2)
    arr = _carray(cs)
    addr = ctypes.addressof(arr)
    cost = np.full(2, 7.0)
    tour = np.full((2, 6), 7, dtype=np.int32)
    junk = 0x1000  # never dereferenced
    for nn, nb in ((0, 2), (21, 2), (5, -1)):
        assert L.tspgpu_distance_matrix_device(h, junk, nn, nb, junk, None) == EINVAL
    for nn, nb in ((1, 2), (21, 2), (5, -1)):
        assert L.tspgpu_solve_cities_device(h, junk, nn, nb, junk, junk, junk, None) == EINVAL
        assert L.tspgpu_solve_cities_upload(h, arr, nn, nb, tspgpu._dp(cost), tspgpu._ip(tour)) == EINVAL
    assert L.tspgpu_distance_matrix_device(h, None, 5, 2, junk, None) == EINVAL
    assert L.tspgpu_distance_matrix_device(h, junk, 5, 2, None, None) == EINVAL
    for hole in range(4):
        ptrs = [junk] * 4
        ptrs[hole] = None
        assert L.tspgpu_solve_cities_device(h, ptrs[0], 5, 2, ptrs[1], ptrs[2], ptrs[3], None) == EINVAL
    assert L.tspgpu_solve_cities_upload(h, None, 5, 2, tspgpu._dp(cost), tspgpu._ip(tour)) == EINVAL
    assert L.tspgpu_solve_cities_upload(h, arr, 5, 2, None, tspgpu._ip(tour)) == EINVAL
    assert L.tspgpu_solve_cities_upload(h, arr, 5, 2, tspgpu._dp(cost), None) == EINVAL
    assert L.tspgpu_distance_matrix_device(h, None, 5, 0, None, None) == 0
    assert L.tspgpu_solve_cities_device(h, None, 5, 0, None, None, None, None) == 0
    assert L.tspgpu_solve_cities_upload(h, None, 5, 0, None, None) == 0
    assert addr and (cost == 7.0).all() and (tour == 7).all()
    with tspgpu.Context(device=0, strict=True) as strict:
        assert L.tspgpu_solve_cities_device(strict.handle, junk, 17, 2, junk, junk, junk, None) == EINVAL
        assert L.tspgpu_solve_cities_upload(strict.handle, arr, 17, 2, tspgpu._dp(cost), tspgpu._ip(tour)) == EINVAL


# 5 -----------------------------------------------------------------------------------------------

MS = re.compile(r"^TSP ran in \d+ ms ", re.M)


@pytest.mark.parametrize("args", [(16, 64, 1000, 1000), (12, 4, 1000, 1000)], ids=["16-64", "12-4"])
def test_cli_device_distances_print_the_same(args):
    """TSP_DEVICE_DIST=1 bin/tsp: stdout identical to the default path (the
    measured milliseconds aside), and TSP_STATS names where the distances ran."""
    env = dict(os.environ, TSP_NPROCS="1", TSP_STATS="1")
    for k in ("PMI_SIZE", "PMI_RANK", "OMPI_COMM_WORLD_SIZE", "OMPI_COMM_WORLD_RANK", "TSP_DEVICE_DIST"):
        env.pop(k, None)
    cmd = [tspgpu.TSP_BIN, *map(str, args)]
    host = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    dev = subprocess.run(cmd, capture_output=True, text=True, env=dict(env, TSP_DEVICE_DIST="1"), timeout=300)
    assert host.returncode == 0 and dev.returncode == 0, host.stderr + dev.stderr
    assert "trip cost" in host.stdout
    assert MS.sub("TSP ran in <ms> ms ", dev.stdout) == MS.sub("TSP ran in <ms> ms ", host.stdout)
    assert re.search(r"distances [0-9.]+ ms of it on the host;", host.stderr), host.stderr
    assert re.search(r"distances [0-9.]+ ms of it on the device;", dev.stderr), dev.stderr


# 6 -----------------------------------------------------------------------------------------------

def test_caller_stream_behind_a_queued_k1_launch(gpu_ctx):
    """The build shares the context's buffers with K1: on a caller stream it
    waits for the launch queued before it on the context's stream."""
    n, B = 16, 512
    cs = _generated(n, B)
    host = _host_dist(cs)
    want_cost, want_tour = gpu_ctx.solve_cities((_carray(cs), n, B))
    other = Shard(n, 2048, 0, 2048).distances()
    d_o, c_o, t_o = gpu_ctx.upload(other), gpu_ctx.alloc(2048 * 8), gpu_ctx.alloc(2048 * (n + 1) * 4)
    s = gpu_ctx.stream_create()
    try:
        gpu_ctx.solve_device(d_o, n, 2048, c_o, t_o, gpu_ctx.stream)
        got = _device_dist(gpu_ctx, cs, stream=s)
        gpu_ctx.solve_device(d_o, n, 2048, c_o, t_o, gpu_ctx.stream)
        cost, tour, status = _solve_device(gpu_ctx, cs, stream=s)
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.synchronize()
        gpu_ctx.synchronize(s)
        gpu_ctx.stream_destroy(s)
        for p in (d_o, c_o, t_o):
            gpu_ctx.free(p)
    assert _same_bits(got, host)
    assert not status.any() and _same_bits(cost, want_cost) and np.array_equal(tour, want_tour)
