"""K1-wide (csrc/hkwide_impl.h) above 22 cities: every push kernel T = 21 .. 29
in both value types, table offsets past 2^32 bytes (n = 27 f64, n = 28 int32)
and past 2^31 / 2^32 elements (n = 29 / n = 30), the uncached workspace for
tables over 1 GB, and the pull form at these sizes.

Up to n = 26 the expected cost and tour are the CPU oracle's
(tests/golden/wide_large.json; tests/test_wide_golden.py ties the file to the
oracle).  Past that they are K2's, an independent exact algorithm, on a run
that did not fall back to K1-wide itself.  Every comparison is on bits and
whole tours.

One answer reads one path through the table, so a layer kernel that is wrong
for some member of its row shows only on an instance whose optimal path takes
that member (measured: with wide_push skipping its last member at T >= 21,
every comparison above passed but one).  test_pinned_tours therefore makes a
known optimum unique and relabels it so that the path takes the last (or the
first) member at every layer; test_relabelling_keeps_the_cost samples others.

n = 31 runs once per value type (a 129 GB / 65 GB table whose allocation
dominates the test), so the "same integers as doubles" cross-check stops at
n = 30.
"""
import ctypes

import numpy as np
import pytest

import oracle_py as O
import tspgpu

pytestmark = pytest.mark.gpu

GOLDEN = O.load_golden("wide_large.json")
GOLDEN_NS = sorted({i["n"] for i in GOLDEN})
GIB = 1 << 30


def table_bytes(n, itemsize):
    """N * 2^(N-1) values, N = n - 1 inner cities."""
    return (n - 1) * 2 ** (n - 2) * itemsize


def free_device_bytes():
    """hipMemGetInfo of the HIP runtime libtspgpu itself runs on: the symbol is
    looked up through libtspgpu's handle, so it resolves in the runtime that
    library is linked against.  (torch carries a HIP runtime of its own, which
    other tests may have brought into this process; it is not the one that
    holds this library's device state, and tests/test_gpu_parity.py keeps
    torch's device calls out of a process that has loaded libtspgpu.)"""
    L = tspgpu.lib()
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.hipSetDevice(ctypes.c_int(0)) == 0
    assert L.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def left_fold(d, tour):
    """((d[0][t1] + d[t1][t2]) + ...) + d[t_{n-1}][0] in d's own arithmetic:
    how the DP accumulates the cost of the tour it returns."""
    acc = d[tour[0], tour[1]]
    for a, b in zip(tour[1:-1], tour[2:]):
        acc = acc + d[a, b]
    return acc


def assert_permutation(tour, n):
    assert len(tour) == n + 1 and tour[0] == 0 and tour[-1] == 0
    assert sorted(tour[1:-1]) == list(range(1, n))


# ---- a. the oracle's goldens, both forms, both types ----

def golden_matrix(inst):
    if inst["kind"] == "integer":
        return np.array(inst["matrix"], dtype=np.int32)
    return tspgpu.distance_matrix([[(c, O.hexf(x), O.hexf(y)) for c, x, y in inst["cities"]]])[0]


@pytest.mark.parametrize("form", ["0", "1"], ids=["push", "pull"])
@pytest.mark.parametrize("n", GOLDEN_NS)
def test_goldens(gpu_ctx, knobs, n, form):
    """wide_push T = 21 .. n - 2 (and wide_layer s up to n - 1) against the CPU
    oracle: uniform cities, a tie-heavy lattice, an asymmetric integer matrix
    in f64 and in int32."""
    assert {23, 24, 25} <= set(GOLDEN_NS)
    knobs.set("WIDE_PULL", form)
    insts = [i for i in GOLDEN if i["n"] == n]
    assert sorted(i["kind"] for i in insts) == ["integer", "lattice", "uniform"]
    for inst in insts:
        d = golden_matrix(inst)
        want = (O.hexf(inst["cost_hex"]), inst["tour"])
        cost, tour, _ = gpu_ctx.solve_instance(d.astype(np.float64))
        assert (cost, tour.tolist()) == want, (n, inst["kind"], "f64", form)
        if inst["kind"] == "integer":
            cost, tour, _ = gpu_ctx.solve_instance_i32(d)
            assert (float(cost), tour.tolist()) == want, (n, "i32", form)


# ---- b. past the oracle: against K2 and against itself ----

SEED = 5
_INSTANCE = {}
_K2 = {}


def large_instance(n, dtype):
    """Uniform cities as bench.k2_instance; int32: those distances times 1000,
    rounded (accidental ties stay rare, n * max(d) ~ 4.4e7 << INT_MAX)."""
    from bench import k2_instance

    if n not in _INSTANCE:
        d = np.asarray(k2_instance(n, SEED))
        di = np.rint(1000 * d).astype(np.int32)
        for m in (d, di):
            m.setflags(write=False)
        _INSTANCE[n] = {"f64": d, "i32": di}
    return _INSTANCE[n][dtype]


def k2_answer(ctx, n, dtype):
    """K2's (cost, tour) on large_instance(n, dtype), searched once; never a
    fallback, which would be K1-wide's own answer."""
    if (n, dtype) not in _K2:
        cost, tour, st = tspgpu.search_solve(ctx, large_instance(n, dtype))
        assert st["fallback"] == 0, (n, dtype, st)
        _K2[(n, dtype)] = (cost, tour.tolist())
    return _K2[(n, dtype)]


def solve(ctx, d):
    """K1-wide in d's own type -> (cost, tour list)"""
    if d.dtype == np.int32:
        cost, tour, _ = ctx.solve_instance_i32(d)
        assert isinstance(cost, int)
    else:
        cost, tour, _ = ctx.solve_instance(d)
    return cost, tour.tolist()


def check_large(ctx, n, dtype):
    d = large_instance(n, dtype)
    want = k2_answer(ctx, n, dtype)
    cost, tour = solve(ctx, d)
    assert (cost, tour) == want, (n, dtype)
    assert_permutation(tour, n)
    fold = left_fold(d, tour)
    assert (int(fold) == cost) if dtype == "i32" else (float(fold).hex() == float(cost).hex()), (n, dtype, fold, cost)
    return cost, tour


# n: the first size with f64 byte offsets past 2^32 (27), element offsets past
# 2^31 (29) and 2^32 (30); the pull form at the first two
LARGE = [(27, "0"), (27, "1"), (29, "0"), (29, "1"), (30, "0")]
LARGE_IDS = [f"n{n}-{'pull' if f == '1' else 'push'}" for n, f in LARGE]


@pytest.mark.parametrize("n,form", LARGE, ids=LARGE_IDS)
def test_large_f64_agrees_with_k2(gpu_ctx, knobs, n, form):
    knobs.set("WIDE_PULL", form)
    check_large(gpu_ctx, n, "f64")


@pytest.mark.parametrize("n,form", LARGE, ids=LARGE_IDS)
def test_large_i32_agrees_with_k2_and_with_f64(gpu_ctx, knobs, n, form):
    knobs.set("WIDE_PULL", form)
    cost, tour = check_large(gpu_ctx, n, "i32")
    c64, t64 = solve(gpu_ctx, large_instance(n, "i32").astype(np.float64))
    assert c64 == float(cost) and t64 == tour


def test_31_cities_i32(gpu_ctx, knobs):
    """wide_push<int32_t, 29>, a 65 GB table."""
    knobs.set("WIDE_PULL", "0")
    check_large(gpu_ctx, 31, "i32")


def test_31_cities_f64(gpu_ctx, knobs):
    """wide_push<double, 29>, a 129 GB table: the one case that may skip, and
    only for want of device memory."""
    knobs.set("WIDE_PULL", "0")
    need = table_bytes(31, 8) + GIB
    free = free_device_bytes()
    if free < need:
        pytest.skip(f"n = 31 f64 needs {need} bytes of device memory (a {table_bytes(31, 8)}-byte table plus 1 GiB), "
                    f"{free} are free")
    check_large(gpu_ctx, 31, "f64")


# ---- c. relabelling invariance ----

@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("dtype", ["i32", "f64"])
@pytest.mark.parametrize("n", [27, 29])
def test_relabelling_keeps_the_cost(gpu_ctx, n, dtype, k):
    """One answer touches only the table entries on its own optimal path; the
    same integer matrix under four relabellings of cities 1 .. n-1 walks
    others.  The sums are exact, so the cost cannot move (all four equal the
    unrelabelled cost); the tour may (the tie rule reads the labels) but must
    fold, mapped back, to that cost."""
    d = large_instance(n, "i32")
    want = k2_answer(gpu_ctx, n, "i32")[0]
    p = np.concatenate(([0], 1 + np.random.default_rng([3100, n, k]).permutation(n - 1)))
    dp = np.ascontiguousarray(d[np.ix_(p, p)])
    cost, tour = solve(gpu_ctx, dp if dtype == "i32" else dp.astype(np.float64))
    assert cost == want, (n, dtype, p.tolist())
    assert_permutation(tour, n)
    assert int(left_fold(d, p[tour])) == want, (n, dtype, p.tolist())


# ---- the optimal path pinned to the ends of every row ----

def golden_integer(n):
    inst = next(i for i in GOLDEN if i["n"] == n and i["kind"] == "integer")
    return np.array(inst["matrix"], dtype=np.int32), int(O.hexf(inst["cost_hex"])), inst["tour"]


def pinned(d, tour, order, seed):
    """d plus a penalty in 1 .. 1000 on every directed edge that `tour` does
    not use, relabelled so that the tour reads 0, 1, .., n-1, 0 ("up") or
    0, n-1, .., 1, 0 ("down") -> (matrix, that tour).

    No tour got cheaper and `tour` kept its cost, so if it was optimal it
    still is, at the same cost, and it is now the only one: any other tour
    uses a penalised edge.  Labelled "up", the DP's optimal path takes the
    LAST member of the row (and the highest destination slot) at every layer;
    labelled "down", the first member and slot 0.  Whatever a layer kernel
    gets wrong at either end of its row is on the one path the answer reads."""
    n = d.shape[0]
    a = np.random.default_rng(seed).integers(1, 1001, size=(n, n)).astype(np.int32)
    np.fill_diagonal(a, 0)
    a[tour[:-1], tour[1:]] = 0
    p = np.array(tour[:-1] if order == "up" else tour[:1] + tour[-2:0:-1])
    want = list(range(n)) + [0] if order == "up" else [0] + list(range(n - 1, 0, -1)) + [0]
    return np.ascontiguousarray((d + a)[np.ix_(p, p)]), want


PINNED = [(n, "0") for n in GOLDEN_NS + [27, 29, 30]] + [(n, "1") for n in GOLDEN_NS + [27, 29]]


@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("dtype", ["i32", "f64"])
@pytest.mark.parametrize("n,form", PINNED, ids=[f"n{n}-{'pull' if f == '1' else 'push'}" for n, f in PINNED])
def test_pinned_tours(gpu_ctx, knobs, n, form, dtype, order):
    """The integer instances whose optimum is known (the oracle's to n = 26,
    K2's past it), with that optimum made unique and labelled up or down."""
    knobs.set("WIDE_PULL", form)
    if n in GOLDEN_NS:
        d, cost, tour = golden_integer(n)
    else:
        d, (cost, tour) = large_instance(n, "i32"), k2_answer(gpu_ctx, n, "i32")
    dp, want = pinned(d, tour, order, [3300, n])
    got = solve(gpu_ctx, dp if dtype == "i32" else dp.astype(np.float64))
    assert got == (cost, want), (n, form, dtype, order)


@pytest.mark.parametrize("order", ["up", "down"])
def test_pinned_tours_31_cities_i32(gpu_ctx, knobs, order):
    """wide_push<int32_t, 29> at either end of its row."""
    knobs.set("WIDE_PULL", "0")
    cost, tour = k2_answer(gpu_ctx, 31, "i32")
    dp, want = pinned(large_instance(31, "i32"), tour, order, [3300, 31])
    assert solve(gpu_ctx, dp) == (cost, want)


# ---- d. workspace lifetime across the 1 GB line ----

def test_workspace_lifetime_across_the_cache_limit(gpu_ctx):
    """A cached small table, then two uncached 27-city ones (each frees what
    was cached and is freed after its call), then small ones again: right
    answers throughout and no table left behind."""
    rng = np.random.default_rng(3200)
    d12 = np.rint(1000 * np.asarray(O.distance_matrix(
        [(i, x, y) for i, (x, y) in enumerate(rng.uniform(0, 1000, size=(12, 2)))]))).astype(np.int32)
    small = O.solve_block(d12.astype(np.float64))
    big64, big32 = k2_answer(gpu_ctx, 27, "f64"), k2_answer(gpu_ctx, 27, "i32")
    free_device_bytes()
    ctx = tspgpu.Context(device=0)
    try:
        assert ctx.wide_last_dtype() == -1
        cost, tour = solve(ctx, d12.astype(np.float64))
        assert (cost, tour) == small and ctx.wide_last_dtype() == tspgpu.F64
        before = free_device_bytes()
        assert solve(ctx, large_instance(27, "f64")) == big64 and ctx.wide_last_dtype() == tspgpu.F64
        assert solve(ctx, large_instance(27, "i32")) == big32 and ctx.wide_last_dtype() == tspgpu.I32
        after = free_device_bytes()
        # a leaked table would cost all of table_bytes(27, 8) (or half of it, the int32 one)
        assert before - after <= table_bytes(27, 8) // 2, (before, after)
        cost, tour = solve(ctx, d12.astype(np.float64))
        assert (cost, tour) == small and ctx.wide_last_dtype() == tspgpu.F64
        cost, tour = solve(ctx, d12)
        assert (float(cost), tour) == small and ctx.wide_last_dtype() == tspgpu.I32
    finally:
        ctx.close()
