"""K1 where a workgroup solves more than one block and a launch is more than
one chunk, every layer kernel the library compiles, and the inputs at the
edge of what tspgpu_validate accepts — each block bit for bit against the
CPU oracle:

  A. variant 6 (hk_sub.h): the forward kernel's persistent loop and the
     backtracking kernel's loop (hk_tiled.h) both run at least three times;
  B. launches split into chunks (k1_launch.cpp ensure_slots; knob K1_CHUNK),
     the product's 65536-block chunk included;
  C. the `slots` option: the global-table layer kernels reuse three slots
     (and their LDS end layers), the LDS-table kernels loop over a batch of
     more than twice their grid;
  D. one case per launch_n instantiation listed in csrc/k1l/hkl_units.h,
     reached through the knobs K1, THREADS and LDS_TABLE_MAX_N;
  E. distances next to the n * max(d) < INT_MAX limit, tiny and subnormal
     ones, negative zeros (refused), and the batch size at which the
     dispatch changes from variant 2 to variant 6.

Large batches are tiled from a few distinct matrices (tiled()), so the oracle
solves each distinct matrix once.  Costs are compared by their bits, tours as
lists; nothing here has a tolerance.
"""
import errno
import os
import re

import numpy as np
import pytest

import tspgpu
from test_k1_variants_gpu import _ctx, _k1_cfgs, _oracle_all

pytestmark = pytest.mark.gpu

F64, I32 = np.float64, np.int32
INT_MAX = 2147483647


# ---------------------------------------------------------------- helpers

def _euclid(xy):
    n = len(xy)
    return tspgpu.distance_matrix([[(i, xy[i, 0], xy[i, 1]) for i in range(n)]])[0]


def _one_matrix(rng, n, cls):
    if cls == 0:
        return _euclid(rng.integers(0, 4, size=(n, 2)).astype(F64))  # tie-heavy lattice
    if cls == 1:
        return _euclid(rng.integers(0, 40, size=(n, 2)).astype(F64))
    if cls == 2:
        return _euclid(rng.uniform(0, 1000, size=(n, 2)))
    if cls == 3:
        m = rng.uniform(0, 1000, (n, n))  # asymmetric, non-integer
    else:
        m = rng.integers(0, 4, size=(n, n)).astype(F64)  # asymmetric and tie-heavy at once
    np.fill_diagonal(m, 0.0)
    return m


def mixed_blocks(n, D, seed, dtype=F64):
    """D distinct n x n matrices cycling through five classes: two integer
    lattices (coordinates 0..3 and 0..39), uniform Euclidean, asymmetric
    non-integer, asymmetric small integers.  int32: the same, rounded."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    for b in range(D):
        for _ in range(64):  # (tiny n: a class may not hold enough different matrices; then a repeat stays)
            m = _one_matrix(rng, n, b % 5)
            if dtype == I32:
                m = np.rint(m)
            if m.tobytes() not in seen:
                break
        seen.add(m.tobytes())
        out.append(m)
    return np.ascontiguousarray(np.array(out), dtype=dtype)


def tiled(distinct, B, seed):
    """A batch of B rows drawn from the distinct matrices -> (batch, source
    index of every row): row b must come out as the oracle's answer for
    distinct[src[b]]."""
    src = np.random.default_rng(seed).integers(0, distinct.shape[0], B)
    return np.ascontiguousarray(distinct[src]), src


def _reference(key, distinct):
    """(cost bits (uint64; exact integers for int32), tours) of the oracle on
    every distinct matrix (int32 matrices converted to double)."""
    res = _oracle_all(("persistent",) + key, distinct.astype(F64))
    n = distinct.shape[1]
    cost = np.array([r[0] for r in res], dtype=F64)
    tours = np.array([r[1] for r in res], dtype=np.int32).reshape(len(res), tspgpu.tour_length(n))
    if distinct.dtype == I32:
        assert np.array_equal(cost, np.rint(cost))
        bits = cost.astype(np.int64)
    else:
        bits = cost.view(np.uint64).copy()
    bits.setflags(write=False)
    tours.setflags(write=False)
    return bits, tours


_SETS = {}


def _distinct(n, dtype):
    """The shared distinct set of a size and type with its oracle answers:
    96 matrices up to 16 cities, 7 above."""
    key = (n, np.dtype(dtype).name)
    if key not in _SETS:
        d = mixed_blocks(n, 96 if n <= 16 else 7, 9000 + n, dtype)
        d.setflags(write=False)
        _SETS[key] = (d, _reference(key, d))
    return _SETS[key]


def _solve(ctx, d):
    return ctx.solve_blocks(d) if d.dtype == F64 else ctx.solve_blocks_i32(d)


def _bits(cost):
    return cost.view(np.uint64) if cost.dtype == F64 else cost.astype(np.int64)


def _compare(got, ref, src=None):
    """Every row of a solve_blocks result against the oracle's bits and tour."""
    cost, tour = got
    rbits, rtour = ref
    if src is not None:
        rbits, rtour = rbits[src], rtour[src]
    L = rtour.shape[1]
    bad = np.flatnonzero((_bits(cost) != rbits) | (tour[:, :L] != rtour).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {cost.shape[0]} blocks differ from the oracle, first {bad[:5].tolist()}"
    assert (tour[:, L:] == -1).all()


def _open(knobs, slots=0, **values):
    """A context created under the given knobs (K1 knobs are read at context
    creation), the knobs cleared again before anything else runs."""
    try:
        for k, v in values.items():
            knobs.set(k, v)
        return tspgpu.Context(device=0, slots=slots)
    finally:
        knobs.clear()


# ------------------------------------------- A. variant 6's persistent loops

B_LOOP = 2 * 6144 + 37


@pytest.mark.parametrize("variant,cfg,vb,n", _k1_cfgs())
def test_forward_and_backtracking_loops_run_three_times(variant, cfg, vb, n):
    dist, ref = _distinct(n, F64 if vb == 8 else I32)
    d, src = tiled(dist, B_LOOP, 100 + cfg)
    ctx = _ctx(None, cfg)  # (the dispatch's own choice of variant, this configuration of it)
    try:
        cu = ctx.device_info()[0]
        got = _solve(ctx, d)
        assert ctx.last_variant() == variant == 6
        assert B_LOOP > 2 * ctx.last_grid()
        # the backtracking grid (k1_launch.cpp solve_sub): TSPGPU_TILED_BTWG = 6 workgroups
        # per CU of kTiledBtWaves = 4 waves, a block per wave (hk_tiled.h)
        assert B_LOOP > 2 * cu * 6 * 4
        _compare(got, ref, src)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [F64, I32], ids=["f64", "i32"])
def test_one_workgroup_per_cu_loops_over_a_small_batch(knobs, dtype):
    dist, ref = _distinct(16, dtype)
    d, src = tiled(dist, 520, 7)
    ctx = _open(knobs, WG_PER_CU=1)
    try:
        got = _solve(ctx, d)
        assert ctx.last_variant() == 6 and ctx.last_grid() == ctx.device_info()[0]
        assert 520 > 2 * ctx.last_grid()
        _compare(got, ref, src)
    finally:
        ctx.close()


# ------------------------------------------------- B. multi-chunk launches

@pytest.mark.parametrize("chunk,B", [(100, 300), (100, 301), (64, 300)])
@pytest.mark.parametrize("n,dtype", [(16, F64), (13, F64), (16, I32)], ids=["n16-f64", "n13-f64", "n16-i32"])
def test_chunked_launch(gpu_ctx, knobs, n, dtype, chunk, B):
    """Three full chunks, a one-block last chunk, a partial last chunk: blocks
    of a later chunk use slot blk - blk0 but cost and tour row blk."""
    dist, ref = _distinct(n, dtype)
    d, src = tiled(dist, B, 1000 + B + chunk)
    one = _solve(gpu_ctx, d)
    assert gpu_ctx.last_variant() == 6
    ctx = _open(knobs, K1_CHUNK=chunk)
    try:
        timed = (chunk, B) == (100, 300)
        if timed:
            ctx.k1_split_timing(True)
        got = _solve(ctx, d)
        assert ctx.last_variant() == 6
        _compare(got, ref, src)
        assert np.array_equal(_bits(got[0]), _bits(one[0])) and np.array_equal(got[1], one[1])
        if timed:  # (the split times sum over the chunks)
            fw, bt = ctx.k1_last_split_ms()
            assert fw > 0 and bt > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("value", [0, -5])
def test_chunk_knob_below_one_is_ignored(gpu_ctx, knobs, value):
    dist, ref = _distinct(13, F64)
    d, src = tiled(dist, 300, 5)
    ctx = _open(knobs, K1_CHUNK=value)
    try:
        got = _solve(ctx, d)
        assert ctx.last_variant() == 6
        _compare(got, ref, src)
    finally:
        ctx.close()


def test_product_chunk_limit_is_crossed():
    """No knob: 65536 + 3 blocks of 13 cities.  Whatever chunk ensure_slots
    settles on, block 65536 and the ones after it are in a later chunk."""
    dist, ref = _distinct(13, F64)
    d, src = tiled(dist, 65536 + 3, 65536)
    ctx = _ctx()
    try:
        got = _solve(ctx, d)
        assert ctx.last_variant() == 6
        _compare(got, ref, src)
    finally:
        ctx.close()


# ----------------------------------- C. `slots` and the layer kernels' loops

def _global_cases():
    out = [(n, dtype, 2 if 13 <= n <= 16 else None) for n in range(11, 21) for dtype in (F64, I32)]
    return out + [(16, F64, 4)]


@pytest.mark.parametrize("n,dtype,k1", _global_cases(),
                         ids=[f"n{n}-{np.dtype(t).name}-k1_{k}" for n, t, k in _global_cases()])
def test_global_table_kernels_reuse_three_slots(knobs, n, dtype, k1):
    """Context(slots=3): three workgroups, each solving several blocks on one
    slot (and one set of LDS end layers)."""
    dist, ref = _distinct(n, dtype)
    B = 11 if n <= 16 else 7
    ctx = _open(knobs, slots=3, **({} if k1 is None else {"K1": k1}))
    try:
        got = _solve(ctx, dist[:B])
        assert ctx.last_grid() == 3 and ctx.last_variant() == (4 if k1 == 4 else 2)
        _compare(got, (ref[0][:B], ref[1][:B]))
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [F64, I32], ids=["f64", "i32"])
@pytest.mark.parametrize("n", [3, 6, 10])
def test_lds_table_kernels_loop(gpu_ctx, n, dtype):
    """The LDS-table kernels' grid is min(B, CUs x (160 KiB / LDS bytes)): at
    3 and 6 cities that is 59 / 61 and 45 / 53 workgroups per CU (f64 / i32;
    heldkarp_impl.h lds_bytes), so the batch there is 40009 blocks."""
    dist, ref = _distinct(n, dtype)
    B = 20011 if n == 10 else 40009
    d, src = tiled(dist, B, 300 + n)
    got = _solve(gpu_ctx, d)
    assert gpu_ctx.last_variant() == 2
    assert B > 2 * gpu_ctx.last_grid()
    _compare(got, ref, src)


def test_slots_does_not_apply_to_the_lds_table_kernels(knobs):
    """include/tspgpu.h: `slots` sizes the global-table kernels' grid only."""
    dist, ref = _distinct(6, F64)
    ctx = _open(knobs, slots=3)
    try:
        got = _solve(ctx, dist[:50])
        assert ctx.last_grid() == 50
        _compare(got, (ref[0][:50], ref[1][:50]))
    finally:
        ctx.close()


# ------------------------------------------ D. every compiled layer kernel

def _layer_units():
    """(type, N, lds, threads, var) of every launch_n instantiation in
    csrc/k1l/hkl_units.h."""
    path = os.path.join(os.path.dirname(tspgpu.PKG_DIR), "tsp-mpi-reduction_amd", "csrc", "k1l", "hkl_units.h")
    rows = [(m.group(1), int(m.group(2)), m.group(3) == "true", int(m.group(4)), int(m.group(5)))
            for m in re.finditer(r"launch_n<(\w+), (\d+), (true|false), (\d+), (\d+)>", open(path).read())]
    # (an empty or partial parse must not quietly run fewer cases)
    assert len(rows) >= 98 and len(set(rows)) == len(rows), len(rows)
    assert {("int32_t", 15, False, 1024, 4), ("double", 11, True, 1024, 1), ("double", 2, False, 256, 2)} <= set(rows)
    return rows


def _unit_knobs(N, lds, threads, var):
    """The knobs that make heldkarp_impl.h launch_threads_v pick this unit."""
    kn = {"K1": 4 if var == 4 else 2}
    if 12 <= N <= 15:
        kn["THREADS"] = threads
    else:
        assert threads == (1024 if lds and N >= 11 else 256)
    if lds:
        assert var == 1 and N <= 11
        if N >= 10:
            kn["LDS_TABLE_MAX_N"] = 11
    else:
        assert var in (2, 4)
        if N <= 9:
            kn["LDS_TABLE_MAX_N"] = 1
    return kn


@pytest.mark.parametrize("vtype,N,lds,threads,var", _layer_units(),
                         ids=[f"{t}-N{N}-{'lds' if l else 'global'}-t{th}-v{v}" for t, N, l, th, v in _layer_units()])
def test_every_compiled_layer_kernel(knobs, vtype, N, lds, threads, var):
    n = N + 1
    dist, ref = _distinct(n, F64 if vtype == "double" else I32)
    B = 11 if N <= 15 else 5
    ctx = _open(knobs, slots=3, **_unit_knobs(N, lds, threads, var))
    try:
        got = _solve(ctx, dist[:B])
        assert ctx.last_variant() == (4 if var == 4 else 2)
        # (which path ran: the LDS-table kernels take a workgroup per block, the others the three slots)
        assert ctx.last_grid() == (B if lds else 3)
        _compare(got, (ref[0][:B], ref[1][:B]))
    finally:
        ctx.close()


# ----------------------------------------------------------- E. edge inputs

def _edge_blocks(kind, n, count=6):
    rng = np.random.default_rng(4242 + 17 * n + len(kind))
    if kind == "i32_limit_equal":
        return np.full((1, n, n), (INT_MAX - 1) // n, dtype=I32)  # every tour ties at the largest legal cost
    if kind == "i32_limit_random":
        return rng.integers(0, (INT_MAX - 1) // n + 1, size=(count, n, n)).astype(I32)
    u = rng.uniform(0, 1, size=(count, n, n))
    for b in range(count):
        np.fill_diagonal(u[b], 0.0)
    if kind == "f64_limit":  # n * max(d) just under INT_MAX, asymmetric, non-integer
        mx = float(INT_MAX) / n
        while n * mx >= float(INT_MAX):
            mx = np.nextafter(mx, 0.0)
        return np.array([m / m.max() * mx for m in u])
    return u * {"f64_tiny": 1e-300, "f64_subnormal": 1e-310}[kind]


_V6 = {(13, "float64"), (14, "float64"), (15, "float64"), (16, "float64"), (16, "int32")}


@pytest.mark.parametrize("n", [5, 13, 16])
@pytest.mark.parametrize("kind", ["f64_limit", "f64_tiny", "f64_subnormal", "i32_limit_equal", "i32_limit_random"])
def test_edge_inputs(gpu_ctx, kind, n):
    """Through the small-batch default (layer kernels) and a 300-block batch
    (variant 6 where the size has it)."""
    dist = _edge_blocks(kind, n)
    if dist.dtype == F64:
        assert tspgpu.validate(dist) == 0
        if kind == "f64_limit":
            assert n * float(dist.max()) > 2147483646.0
        if kind == "f64_subnormal":
            assert 0 < dist.max() < np.finfo(F64).tiny
    else:
        assert tspgpu.validate_i32(dist) == 0
        assert 0.9 * INT_MAX < n * int(dist.max()) < INT_MAX
    ref = _reference(("edge", kind, n), dist)
    if kind != "i32_limit_equal":
        assert len(set(ref[0].tolist())) > 1  # (the costs did not all collapse to one value)
    _compare(_solve(gpu_ctx, dist), ref)
    assert gpu_ctx.last_variant() == 2
    d, src = tiled(dist, 300, n)
    got = _solve(gpu_ctx, d)
    assert gpu_ctx.last_variant() == (6 if (n, dist.dtype.name) in _V6 else 2)
    _compare(got, ref, src)


def _negative_zero_blocks(n):
    a = np.zeros((n, n))
    a[0, 1] = a[1, 2] = -0.0
    c = np.zeros((n, n))
    for i in range(n):
        c[i, (i + 1) % n] = -0.0  # one tour of -0.0 edges: the kernels return -0.0, the oracle +0.0
    return [a, np.full((n, n), -0.0), c]


@pytest.mark.parametrize("n", [5, 13, 16])
def test_solve_blocks_refuses_negative_zero(gpu_ctx, n):
    """A minimum over zeros of both signs has no sign the kernels (v_min_f64)
    and the reference (strict <) agree on, so -0.0 is not a valid distance:
    alone, and as one block among 300 valid ones."""
    good, ref = _distinct(n, F64)
    for m in _negative_zero_blocks(n):
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.solve_blocks(m[None])
        assert e.value.code == -errno.EINVAL
        d, src = tiled(good, 300, n)
        d[299] = m
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.solve_blocks(d)
        assert e.value.code == -errno.EINVAL
        # (+0.0 in the same places is an ordinary input: all-zero matrix, cost +0.0, the oracle's tour)
        zref = _reference(("zero", n), np.zeros((1, n, n)))
        assert zref[0][0] == 0  # bits of +0.0
        _compare(gpu_ctx.solve_blocks(np.abs(m)[None]), zref)


def test_dispatch_boundary_at_one_block_per_cu(gpu_ctx):
    """16 cities f64: fewer blocks than CUs run the layer kernel, a block per
    CU and more the sub-cube kernel."""
    dist, ref = _distinct(16, F64)
    cu = gpu_ctx.device_info()[0]
    d, src = tiled(dist, cu, 16)
    for B, variant in ((cu - 1, 2), (cu, 6)):
        got = _solve(gpu_ctx, d[:B])
        assert gpu_ctx.last_variant() == variant
        _compare(got, ref, src[:B])
