"""K1-wide on int32 distances (tspgpu_solve_instance_i32, csrc/hkwide_i32.hip):
the same DP, tie rule and tour layout as the f64 K1-wide on an int32 table.

The expected cost and tour always come from the CPU oracle on the matrix
converted to double: n * max(d) < INT_MAX keeps every partial sum an exact
integer below 2^31, so the f64 DP and the int32 DP take identical decisions
(how tests/test_i32_gpu.py pins K1 on int32).  Bit-exact on cost and tour.
"""
import errno

import numpy as np
import pytest

import oracle_py as O
import tspgpu

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
_ORACLE = {}


def oracle(d):
    """(cost, tour) of the CPU oracle on double(d), computed once per matrix."""
    key = (d.shape[0], d.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = O.solve_block(d.astype(np.float64))
    return _ORACLE[key]


def rounded_euclid(xy):
    m = np.rint(np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])).astype(np.int32)
    np.fill_diagonal(m, 0)
    return m


def matrix(rng, n, kind):
    if kind == "lattice":  # rounded Euclidean on lattice coordinates 0..3: tie-heavy
        return rounded_euclid(rng.integers(0, 4, size=(n, 2)).astype(np.float64))
    if kind == "uniform":  # rounded Euclidean on uniform coordinates (TSPLIB EUC_2D)
        return rounded_euclid(rng.uniform(0, 1000, size=(n, 2)))
    hi = 1_000_000 if kind == "asym_wide" else 4
    m = rng.integers(0, hi, size=(n, n)).astype(np.int32)
    np.fill_diagonal(m, 0)
    return m


def check(ctx, d):
    cost, tour, _ = ctx.solve_instance_i32(d)
    oc, ot = oracle(d)
    assert isinstance(cost, int) and tour.dtype == np.int32
    assert float(cost) == oc and tour.tolist() == ot, (d.shape[0], cost, oc, tour.tolist(), ot)
    return cost, tour


@pytest.mark.parametrize("n", [3, 4, 6, 10, 14, 17, 20])
def test_oracle_k1_and_f64_agree(gpu_ctx, n):
    """n = 3: one push layer; 4: the first real min; 14: the first with more
    rows than one 256-thread block in the middle layers (C(13,6) = 1716); 17
    and 20 straddle the pull/push default."""
    rng = np.random.default_rng(7100 + n)
    kinds = ["lattice", "uniform", "asym_wide", "asym_small"]
    for kind in kinds if n < 17 else kinds[:2]:
        d = matrix(rng, n, kind)
        cost, tour = check(gpu_ctx, d)
        c1, t1 = gpu_ctx.solve_blocks_i32(d[None])
        assert int(c1[0]) == cost and t1[0].tolist() == tour.tolist(), (n, kind)
        c64, t64, _ = gpu_ctx.solve_instance(d.astype(np.float64))
        assert c64 == float(cost) and t64.tolist() == tour.tolist(), (n, kind)


@pytest.mark.parametrize("form", ["0", "1"])
def test_push_and_pull_forms(gpu_ctx, form, knobs):
    """Both layer forms (row-owner push, per-destination pull) at every size,
    on the same instances (the oracle runs once per instance)."""
    knobs.set("WIDE_PULL", form)
    rng = np.random.default_rng(7177)
    for n in (3, 5, 9, 13, 16, 18, 20):
        for kind in ("lattice", "uniform"):
            check(gpu_ctx, matrix(rng, n, kind))


@pytest.mark.parametrize("n", [21, 22])
def test_beyond_k1_agrees_with_k2(gpu_ctx, n):
    """Past K1's sizes: K2 on int32, an independent exact algorithm."""
    rng = np.random.default_rng(7200 + n)
    d = matrix(rng, n, "uniform")
    cost, tour, _ = gpu_ctx.solve_instance_i32(d)
    c2, t2, _ = tspgpu.search_solve(gpu_ctx, d)
    assert cost == c2 and tour.tolist() == t2.tolist()


def test_tie_rule_at_the_extreme(gpu_ctx):
    """Every tour optimal: the tour is the tie rule's alone."""
    check(gpu_ctx, np.zeros((13, 13), dtype=np.int32))
    d = np.full((12, 12), 7, dtype=np.int32)
    np.fill_diagonal(d, 0)
    check(gpu_ctx, d)


@pytest.mark.parametrize("n", [5, 12])
def test_range_edge(gpu_ctx, n):
    """Weights just inside n * max(d) < INT_MAX: tour sums reach just under
    2^31 without overflow; one step further is refused."""
    rng = np.random.default_rng(7300 + n)
    top = (INT_MAX - 1) // n
    d = rng.integers(top - 1000, top + 1, size=(n, n)).astype(np.int32)
    np.fill_diagonal(d, 0)
    cost, _ = check(gpu_ctx, d)
    assert INT_MAX - n * 1001 <= cost < INT_MAX
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_instance_i32(np.full((n, n), INT_MAX // n + 1, dtype=np.int32))
    assert e.value.code == -errno.ERANGE
    bad = d.copy()
    bad[n - 1, 1] = -1
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_instance_i32(bad)
    assert e.value.code == -errno.EINVAL


def test_rejects_bad_sizes_and_values_past_20_cities(gpu_ctx):
    for n in (2, 32):
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.solve_instance_i32(np.zeros((n, n), dtype=np.int32))
        assert e.value.code == -errno.EINVAL
    # above tspgpu_validate_i32's 20 cities the entry checks the values itself
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_instance_i32(np.full((25, 25), INT_MAX // 25 + 1, dtype=np.int32))
    assert e.value.code == -errno.ERANGE
    bad = np.ones((25, 25), dtype=np.int32)
    bad[24, 3] = -5
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.solve_instance_i32(bad)
    assert e.value.code == -errno.EINVAL


def test_k2_fallback_stays_integer(gpu_ctx, knobs):
    """Too many tied optima to enumerate (13 coincident cities, the device tie
    rule off): K2 answers through K1-wide of the instance's own value type."""
    knobs.set("SEARCH_TIE", "0")
    d = np.zeros((13, 13), dtype=np.int32)
    cost, tour, st = tspgpu.search_solve(gpu_ctx, d)
    assert st["fallback"] == 1, st
    assert cost == 0 and tour.tolist() == oracle(d)[1]
    assert gpu_ctx.wide_last_dtype() == tspgpu.I32
    cost, tour, st = tspgpu.search_solve(gpu_ctx, np.zeros((13, 13)))
    assert st["fallback"] == 1, st
    assert cost == 0.0 and tour.tolist() == oracle(d)[1]
    assert gpu_ctx.wide_last_dtype() == tspgpu.F64


def test_workspace_keyed_by_type():
    """One context, alternating value types and sizes: a cached table is
    reused only for the same (n, type), never a half-sized one."""
    rng = np.random.default_rng(7400)
    d12, d9 = matrix(rng, 12, "uniform"), matrix(rng, 9, "lattice")
    ctx = tspgpu.Context(device=0)
    try:
        assert ctx.wide_last_dtype() == -1
        for d, dtype in ((d12, "f64"), (d12, "i32"), (d12, "f64"), (d9, "i32"), (d12, "i32"), (d9, "f64")):
            oc, ot = oracle(d)
            if dtype == "i32":
                cost, tour, _ = ctx.solve_instance_i32(d)
                assert ctx.wide_last_dtype() == tspgpu.I32
            else:
                cost, tour, _ = ctx.solve_instance(d.astype(np.float64))
                assert ctx.wide_last_dtype() == tspgpu.F64
            assert float(cost) == oc and tour.tolist() == ot, (d.shape[0], dtype)
    finally:
        ctx.close()
