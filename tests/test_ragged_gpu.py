"""Ragged batches on the GPU (tspgpu_solve_ragged, tspgpu_solve_ragged_device):
blocks of different sizes in one call, every block validated on the device.

Nothing here has a tolerance: costs are compared as bits, tours entry by
entry, and the padding of a tour row must be exactly -1.  The references are
the CPU oracle (solved once per matrix and shared) and the uniform entry points
ctx.solve_blocks / ctx.solve_blocks_i32 on the same matrices.

Sizes: every n from 2 to 20 — n = 2 (4 elements, the two-entry tour), n = 8
(exactly one pass of the gather's 64 lanes), n = 9 (81 elements, a partial
second pass), n = 20 (400 elements, a partial seventh pass)."""
import errno
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_py as O
import tspgpu
from test_k1_bookkeeping_gpu import DISTINCT, _reference as _k1_reference

pytestmark = pytest.mark.gpu

F64, I32 = np.float64, np.int32
EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE


def _kind(rng, n, cls):
    """The three kinds of tests/test_k1_bookkeeping_gpu.py."""
    if cls == 0:
        m = rng.uniform(0, 1000, (n, n))  # asymmetric, non-integer
    elif cls == 1:
        xy = rng.integers(0, 4, size=(n, 2)).astype(F64)  # tie-heavy lattice
        m = tspgpu.distance_matrix([[(i, xy[i, 0], xy[i, 1]) for i in range(n)]])[0]
    else:
        m = rng.integers(0, 4, size=(n, n)).astype(F64)  # asymmetric small integers
    np.fill_diagonal(m, 0.0)
    return np.ascontiguousarray(m)


_CACHE = {}


def _every_size(dtype):
    """(matrices, oracle cost bits, oracle tours): three blocks each of n = 2..16
    and one each of n = 17..20, shuffled with a fixed seed; solved once."""
    key = np.dtype(dtype).name
    if key not in _CACHE:
        rng = np.random.default_rng(8100)
        mats = [_kind(rng, n, cls) for n in range(2, 17) for cls in range(3)]
        mats += [_kind(rng, n, n % 3) for n in range(17, 21)]
        order = np.random.default_rng(8101).permutation(len(mats))
        mats = [mats[i] for i in order]
        if dtype == I32:
            mats = [np.rint(m).astype(I32) for m in mats]
        with ThreadPoolExecutor(max_workers=8) as ex:
            res = list(ex.map(lambda m: O.solve_block(np.asarray(m, dtype=F64)), mats))
        for m in mats:
            m.setflags(write=False)
        bits = [_bits(np.array([c], dtype=F64) if dtype == F64 else np.array([int(c)], dtype=I32))[0] for c, _ in res]
        if dtype == I32:
            assert all(c == int(c) for c, _ in res)
        _CACHE[key] = (mats, bits, [t for _, t in res])
    return _CACHE[key]


def _bits(cost):
    return cost.view(np.uint64) if cost.dtype == F64 else cost.astype(np.int64)


def _pack(mats):
    ns = np.array([m.shape[0] for m in mats], dtype=np.int32)
    off = np.concatenate(([0], np.cumsum(ns.astype(np.int64) ** 2)[:-1])).astype(np.int64)
    flat = np.concatenate([m.ravel() for m in mats])
    return flat, off, ns


def _assert_rows(cost, tours, status, want_bits, want_tours, what=""):
    """Every block solved, its cost bits and tour the wanted ones, the padding -1."""
    assert status.tolist() == [0] * len(want_bits), f"{what}: status {status.tolist()}"
    got = _bits(cost)
    for b, (wb, wt) in enumerate(zip(want_bits, want_tours)):
        wt = list(wt)
        assert int(got[b]) == int(wb), f"{what}: block {b} cost bits {int(got[b]):#x} != {int(wb):#x}"
        assert tours[b, : len(wt)].tolist() == wt, f"{what}: block {b} tour"
        assert (tours[b, len(wt):] == -1).all(), f"{what}: block {b} padding {tours[b].tolist()}"


def _uniform_answers(ctx, mats):
    """Per block (cost bits, tour without padding) from the uniform entry point, one call per size."""
    out = [None] * len(mats)
    for n in sorted({m.shape[0] for m in mats}):
        idx = [i for i, m in enumerate(mats) if m.shape[0] == n]
        d = np.ascontiguousarray(np.array([mats[i] for i in idx]))
        cost, tour = ctx.solve_blocks_i32(d) if d.dtype == I32 else ctx.solve_blocks(d)
        L = tspgpu.tour_length(n)
        assert (tour[:, L:] == -1).all()
        for j, i in enumerate(idx):
            out[i] = (int(_bits(cost)[j]), tour[j, :L].tolist())
    return out


def _assert_refused(cost, tours, status, b, code):
    assert status[b] == code, f"block {b}: status {status[b]} != {code}"
    if cost.dtype == F64:
        assert np.isnan(cost[b]), f"block {b}: cost {cost[b]!r}"
    else:
        assert cost[b] == -1, f"block {b}: cost {cost[b]!r}"
    assert (tours[b] == -1).all(), f"block {b}: tour row {tours[b].tolist()}"


# 1, 2 --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F64, I32], ids=["f64", "int32"])
def test_every_size_matches_the_oracle_and_the_uniform_entry(gpu_ctx, dtype):
    mats, bits, otours = _every_size(dtype)
    cost, tours, status = gpu_ctx.solve_ragged(mats)
    assert cost.dtype == dtype and tours.shape == (len(mats), 21) and tours.dtype == I32
    _assert_rows(cost, tours, status, bits, otours, "oracle")
    assert gpu_ctx.last_variant() == 2  # (the last bucket: one block of 20 cities)
    uni = _uniform_answers(gpu_ctx, mats)
    _assert_rows(cost, tours, status, [u[0] for u in uni], [u[1] for u in uni], "solve_blocks")


# 3 -----------------------------------------------------------------------------------------------

def _small():
    mats, bits, otours = _every_size(F64)
    keep = [i for i, m in enumerate(mats) if m.shape[0] <= 12]
    return [mats[i] for i in keep], [bits[i] for i in keep], [otours[i] for i in keep]


def _gapped(mats):
    """A gap in front of every block that makes its element offset odd; the gaps hold NaN."""
    off, at = [], 0
    for m in mats:
        at += 1 if at % 2 == 0 else 2
        off.append(at)
        at += m.size
    flat = np.full(at, np.nan)
    for o, m in zip(off, mats):
        flat[o:o + m.size] = m.ravel()
    assert all(o % 2 == 1 for o in off)
    return flat, np.array(off, dtype=np.int64)


def test_layouts_give_the_packed_answers(gpu_ctx):
    mats, bits, otours = _small()
    B = len(mats)
    assert B == 33
    flat, off, ns = _pack(mats)
    cost, tours, status = gpu_ctx.solve_ragged_flat(flat, off, ns)
    assert tours.shape == (B, 13)
    _assert_rows(cost, tours, status, bits, otours, "packed")

    # offsets in descending order: the blocks laid out back to front
    rev_flat, rev_off, _ = _pack(mats[::-1])
    got = gpu_ctx.solve_ragged_flat(rev_flat, rev_off[::-1].copy(), ns)
    assert (np.diff(rev_off[::-1]) < 0).all()
    _assert_rows(*got, bits, otours, "descending offsets")

    # an odd gap in front of every block (host form: the gaps travel and are never read as a block)
    gap_flat, gap_off = _gapped(mats)
    got = gpu_ctx.solve_ragged_flat(gap_flat, gap_off, ns)
    _assert_rows(*got, bits, otours, "odd gaps")

    # two blocks share one offset: the second becomes a copy of the first
    i, j = [k for k in range(B) if ns[k] == 9][:2]
    off2 = off.copy()
    off2[j] = off[i]
    want_b, want_t = list(bits), list(otours)
    want_b[j], want_t[j] = bits[i], otours[i]
    got = gpu_ctx.solve_ragged_flat(flat, off2, ns)
    _assert_rows(*got, want_b, want_t, "shared offset")

    # a tour_stride larger than needed
    got = gpu_ctx.solve_ragged_flat(flat, off, ns, tour_stride=17)
    assert got[1].shape == (B, 17)
    _assert_rows(*got, bits, otours, "tour_stride 17")

    # 4k + 1 (all 33), 4k + 2, 4k + 3 blocks and one alone: the last workgroup partly empty
    for count in (1, 5, 6, 7):
        f, o, k = _pack(mats[:count])
        got = gpu_ctx.solve_ragged_flat(f, o, k)
        _assert_rows(*got, bits[:count], otours[:count], f"{count} blocks")


def test_unaligned_sources_on_the_device(gpu_ctx):
    """An odd element offset for every block: no source is 16-byte aligned
    (the device form, so that the offsets are the device addresses')."""
    mats, bits, otours = _small()
    B = len(mats)
    ns = np.array([m.shape[0] for m in mats], dtype=np.int32)
    flat, off = _gapped(mats)
    ctx = gpu_ctx
    ptrs = [ctx.upload(flat), ctx.alloc(8 * B), ctx.alloc(4 * 13 * B), ctx.alloc(4 * B)]
    try:
        assert ptrs[0] % 16 == 0
        ctx.solve_ragged_device(ptrs[0], tspgpu.F64, off, ns, ptrs[1], ptrs[2], 13, ptrs[3], ctx.stream)
        ctx.synchronize()
        got = (ctx.download(ptrs[1], (B,), F64), ctx.download(ptrs[2], (B, 13), I32), ctx.download(ptrs[3], (B,), I32))
    finally:
        for p in ptrs:
            ctx.free(p)
    _assert_rows(*got, bits, otours, "odd offsets")


# 4 -----------------------------------------------------------------------------------------------

SPOIL_N = (5, 8, 9, 13, 16)


def _forty(dtype):
    rng = np.random.default_rng(8400)
    mats = []
    for n in SPOIL_N:
        for _ in range(8):
            m = rng.uniform(1, 1000, (n, n))
            np.fill_diagonal(m, 0.0)
            mats.append(np.rint(m).astype(I32) if dtype == I32 else m)
    order = np.random.default_rng(8401).permutation(len(mats))
    return [mats[i] for i in order]


def _nth(mats, n, k):
    """index of the k-th block of n cities"""
    return [i for i, m in enumerate(mats) if m.shape[0] == n][k]


@pytest.mark.parametrize("dtype", [F64, I32], ids=["f64", "int32"])
def test_bad_blocks_cost_only_themselves(gpu_ctx, dtype):
    clean = _forty(dtype)
    B = len(clean)
    c0, t0, s0 = gpu_ctx.solve_ragged(clean)
    uni = _uniform_answers(gpu_ctx, clean)
    _assert_rows(c0, t0, s0, [u[0] for u in uni], [u[1] for u in uni], "clean run")

    bad = [m.copy() for m in clean]
    want = {}
    if dtype == F64:
        a = _nth(bad, 5, 0); bad[a].flat[0] = np.nan; want[a] = EINVAL
        b = _nth(bad, 16, 1); bad[b].flat[-1] = -np.inf; want[b] = EINVAL
        c = _nth(bad, 9, 0); bad[c].flat[63] = -1.0; want[c] = EINVAL
        d = _nth(bad, 9, 1); bad[d].flat[64] = -0.0; want[d] = EINVAL
        e = _nth(bad, 13, 2); bad[e].flat[7] = 1e300; bad[e].flat[100] = -5.0; want[e] = EINVAL
        f = _nth(bad, 8, 3); bad[f][:] = 2147483647.0 / 8; want[f] = ERANGE
        validate = tspgpu.validate
    else:
        a = _nth(bad, 5, 0); bad[a].flat[0] = -1; want[a] = EINVAL
        b = _nth(bad, 16, 1); bad[b].flat[-1] = -2147483648; want[b] = EINVAL
        c = _nth(bad, 9, 0); bad[c].flat[63] = -1; want[c] = EINVAL
        d = _nth(bad, 9, 1); bad[d].flat[64] = -1; want[d] = EINVAL
        e = _nth(bad, 13, 2); bad[e].flat[7] = 2147483647; bad[e].flat[100] = -5; want[e] = EINVAL
        f = _nth(bad, 8, 3); bad[f][:] = 2147483647 // 8 + 1; want[f] = ERANGE
        validate = tspgpu.validate_i32
    for i, code in want.items():
        assert validate(bad[i][None]) == code  # (the host's verdict on that block alone)
    flat, off, ns = _pack(bad)
    # a block of 21 cities whose offset points outside the array: refused by the plan, never read
    g = _nth(bad, 13, 5)
    ns[g], off[g] = 21, flat.size + 1000
    want[g] = EINVAL
    assert len(want) == 7
    cost, tours, status = gpu_ctx.solve_ragged_flat(flat, off, ns, tour_stride=17)
    for i, code in want.items():
        _assert_refused(cost, tours, status, i, code)
    good = [i for i in range(B) if i not in want]
    assert (status[good] == 0).all()
    assert np.array_equal(_bits(cost)[good], _bits(c0)[good]), "a neighbour's cost changed"
    assert np.array_equal(tours[good], t0[good]), "a neighbour's tour changed"


# 5 -----------------------------------------------------------------------------------------------

def test_strict_context_refuses_17_cities_and_solves_its_neighbours(gpu_ctx):
    mats, _, _ = _every_size(F64)
    m16 = [m for m in mats if m.shape[0] == 16]
    m17 = [m for m in mats if m.shape[0] == 17]
    batch = [m16[0], m17[0], m16[1], m16[2]]
    uni = _uniform_answers(gpu_ctx, [m16[0], m16[1], m16[2]])
    ctx = tspgpu.Context(device=0, strict=True)
    try:
        cost, tours, status = ctx.solve_ragged_flat(*_pack(batch), tour_stride=18)
    finally:
        ctx.close()
    _assert_refused(cost, tours, status, 1, EINVAL)
    keep = [0, 2, 3]
    _assert_rows(cost[keep], tours[keep], status[keep], [u[0] for u in uni], [u[1] for u in uni], "strict")
    # the same batch on a context that is not strict: all four solved
    assert gpu_ctx.solve_ragged(batch)[2].tolist() == [0, 0, 0, 0]


# 6 -----------------------------------------------------------------------------------------------

def test_large_bucket_takes_the_product_kernel(gpu_ctx):
    d, bits16, tours16 = _k1_reference(16, F64)
    cu = gpu_ctx.device_info()[0]
    B16 = 2 * cu + 1
    src = np.random.default_rng(16).integers(0, DISTINCT, B16)
    src[:DISTINCT] = np.arange(DISTINCT)
    rng = np.random.default_rng(8600)
    m7 = [_kind(rng, 7, k % 3) for k in range(50)]
    seven = _uniform_answers(gpu_ctx, m7)
    # the 50 small blocks spread among the large ones
    where = np.sort(np.random.default_rng(8601).choice(B16 + 50, 50, replace=False))
    mats, want_b, want_t, i16, i7 = [], [], [], 0, 0
    for pos in range(B16 + 50):
        if i7 < 50 and pos == where[i7]:
            mats.append(m7[i7]); want_b.append(seven[i7][0]); want_t.append(seven[i7][1]); i7 += 1
        else:
            s = src[i16]; i16 += 1
            mats.append(d[s]); want_b.append(bits16[s]); want_t.append(tours16[s].tolist())
    assert i16 == B16 and i7 == 50
    cost, tours, status = gpu_ctx.solve_ragged_flat(*_pack(mats))
    assert gpu_ctx.last_variant() == 6 and gpu_ctx.last_grid() == B16
    _assert_rows(cost, tours, status, want_b, want_t, "2 x CUs + 1 blocks of 16 cities among 50 of 7")


# 7 -----------------------------------------------------------------------------------------------

def test_call_level_errors(gpu_ctx):
    mats, _, _ = _small()
    flat, off, ns = _pack(mats)
    B = len(mats)
    out = (np.full(B, 7.0), np.full((B, 12), 7, dtype=I32), np.full(B, 7, dtype=I32))
    with pytest.raises(tspgpu.TspGpuError) as ei:
        gpu_ctx.solve_ragged_flat(flat, off, ns, tour_stride=12, out=out)  # the largest n is 12
    assert ei.value.code == EINVAL
    assert (out[0] == 7.0).all() and (out[1] == 7).all() and (out[2] == 7).all()
    # (a refused block's n does not count: 21 cities among them changes nothing)
    ns2 = ns.copy()
    ns2[0] = 21
    out13 = (np.full(B, 7.0), np.full((B, 13), 7, dtype=I32), np.full(B, 7, dtype=I32))
    cost, tours, status = gpu_ctx.solve_ragged_flat(flat, off, ns2, tour_stride=13, out=out13)
    assert status[0] == EINVAL and (status[1:] == 0).all() and cost is out13[0]
    # every block refused by the plan: nothing is read or solved, the call still succeeds
    cost, tours, status = gpu_ctx.solve_ragged_flat(flat, [-1, 0, 5], [5, 1, 21], tour_stride=1)
    assert tours.shape == (3, 1)
    for b in range(3):
        _assert_refused(cost, tours, status, b, EINVAL)
    # an empty batch
    cost, tours, status = gpu_ctx.solve_ragged([])
    assert cost.shape == (0,) and tours.shape[0] == 0 and status.shape == (0,)
    with pytest.raises(tspgpu.TspGpuError) as ei:
        gpu_ctx.solve_ragged_device(0, 7, off, ns, 0, 0, 13, 0)  # unknown dtype
    assert ei.value.code == EINVAL


# 8 -----------------------------------------------------------------------------------------------

def test_device_form_on_a_second_stream_then_k1_on_the_contexts(gpu_ctx):
    """The staging buckets and the K1 workspace are the context's: the K1 launch
    on the context's stream must wait for the ragged call on the other one."""
    ctx = gpu_ctx
    mats = _forty(F64)
    B = len(mats)
    uni = _uniform_answers(ctx, mats)
    flat, off, ns = _pack(mats)
    m13 = np.ascontiguousarray(np.array([m for m in mats if m.shape[0] == 13]))
    k1_cost, k1_tour = ctx.solve_blocks(m13)
    K = m13.shape[0]
    stream = ctx.stream_create()
    ptrs = [ctx.upload(flat), ctx.alloc(8 * B), ctx.alloc(4 * 17 * B), ctx.alloc(4 * B),
            ctx.upload(m13), ctx.alloc(8 * K), ctx.upload(np.full((K, 14), -1, dtype=I32))]
    try:
        ctx.solve_ragged_device(ptrs[0], tspgpu.F64, off, ns, ptrs[1], ptrs[2], 17, ptrs[3], stream)
        ctx.solve_device(ptrs[4], 13, K, ptrs[5], ptrs[6], ctx.stream)
        ctx.synchronize(stream)
        ctx.synchronize()
        got = (ctx.download(ptrs[1], (B,), F64), ctx.download(ptrs[2], (B, 17), I32), ctx.download(ptrs[3], (B,), I32))
        c13, t13 = ctx.download(ptrs[5], (K,), F64), ctx.download(ptrs[6], (K, 14), I32)
    finally:
        ctx.stream_destroy(stream)
        for p in ptrs:
            ctx.free(p)
    _assert_rows(*got, [u[0] for u in uni], [u[1] for u in uni], "ragged on the second stream")
    assert np.array_equal(_bits(c13), _bits(k1_cost)) and np.array_equal(t13, k1_tour)
