"""Ragged blocks from cities to the merged tour (tspgpu_pipeline_cities_ragged,
tspgpu_reduce_ragged_device behind tspgpu_solve_cities_ragged_device,
tspgpu_reduce_ragged): against a Python replay of the
reference's schedule over the oracle's mergeBlocks (which takes two paths of
any length), through near-tie stalls and the fold kernel's LDS hand-over with
blocks of different lengths, the fold_ok decision under four id layouts, the
uniform forms bit for bit on uniform input, the error contract and a caller
stream.  Nothing here has a tolerance."""
import errno
import functools

import numpy as np
import pytest

import tspgpu
from test_host import _solve_all
from test_pipeline_gpu import TWO_CITY, DeviceK1, bits, make_blocks, replay, two_city_blocks

pytestmark = pytest.mark.gpu
EINVAL, ENOSPC = -errno.EINVAL, -errno.ENOSPC


def ragged_blocks(ns, seed, kind="random"):
    """Blocks of ns[b] cities with ids unique across blocks.  lattice: the
    blocks of make_blocks("lattice", 9, B, seed) re-cut to ns[b] cities."""
    if kind == "lattice":
        assert max(ns) <= 9
        full = make_blocks("lattice", 9, len(ns), seed)
        return [blk[:n] for blk, n in zip(full, ns)]
    rng = np.random.default_rng(seed)
    blocks, at = [], 0
    for n in ns:
        xy = rng.uniform(0, 1000, size=(n, 2))
        blocks.append([(at + i, xy[i, 0], xy[i, 1]) for i in range(n)])
        at += n
    return blocks


def expected_log(ns, P):
    """The receive lines of tsp.cpp:88: a rank's folded path has its first
    block's cities and every further block's but the closing copy."""
    B = len(ns)
    cnt = [0] * P
    for b in range(1, B + 1):
        cnt[b % P] += 1
    lens, at = [], 0
    for r in range(P):
        L = [tspgpu.tour_length(n) for n in ns[at:at + cnt[r]]]
        lens.append(L[0] + sum(x - 1 for x in L[1:]))
        at += cnt[r]
    lastpower = 1 << (P.bit_length() - 1)
    return "".join("process %i is about to receive %i cities from process %i\n" % (i, lens[i + lastpower],
                                                                                    i + lastpower)
                   for i in range(P - lastpower))


class RaggedK1:
    """Packed cities uploaded and solved on the device
    (tspgpu_solve_cities_ragged_device): the pointers tspgpu_reduce_ragged_device takes."""

    def __init__(self, ctx, blocks, stream=0, extra_stride=0):
        self.ctx = ctx
        arr, self.ns = tspgpu.cities_array_ragged(blocks)
        self.B = len(self.ns)
        self.stride = int(self.ns.max()) + 1 + extra_stride
        self.total = sum(tspgpu.tour_length(int(n)) for n in self.ns)
        self.ptrs = []
        self.cities = self._keep(ctx.upload(np.frombuffer(arr, dtype=tspgpu.CITY_DTYPE, count=int(self.ns.sum()))))
        self.cost = self._keep(ctx.alloc(8 * self.B))
        self.tour = self._keep(ctx.alloc(4 * self.B * self.stride))
        self.status = self._keep(ctx.alloc(4 * self.B))
        ctx.solve_cities_ragged_device(self.cities, self.ns, self.cost, self.tour, self.stride, self.status, stream)
        self.k1_stream = stream

    _keep = DeviceK1._keep
    path_buffer = DeviceK1.path_buffer
    download_path = DeviceK1.download_path
    poke = DeviceK1.poke
    close = DeviceK1.close

    def reduce(self, P, cap=None, stream=0, status=True, d_path=None):
        """-> (cost, log, path length, downloaded path as (id, x, y) tuples)"""
        if cap is None:
            cap = 6 * self.total + 1
        if d_path is None:
            d_path = self.path_buffer(cap)
        cost, log, plen = self.ctx.reduce_ragged_device(self.cities, self.ns, self.tour, self.stride, self.cost,
                                                        self.status if status else 0, P, d_path, cap, stream)
        return cost, log, plen, self.download_path(d_path, plen)


def host_gather(ctx, blocks):
    """solve_cities_ragged and the host gather (convPathToCityPath) -> (paths, costs)"""
    cost, tour, status = ctx.solve_cities_ragged(blocks)
    assert not status.any()
    paths = [[blk[t] for t in tour[b][:tspgpu.tour_length(len(blk))]] for b, blk in enumerate(blocks)]
    return paths, cost


def three_forms(ctx, blocks, P):
    """pipeline_cities_ragged, reduce_ragged_device behind the device solve, and
    reduce_ragged on the host-gathered paths -> [(cost, log, path)] * 3"""
    out = [ctx.pipeline_cities_ragged(blocks, P)]
    k1 = RaggedK1(ctx, blocks)
    try:
        cost, log, plen, path = k1.reduce(P)
        assert plen == len(path)
        out.append((cost, log, path))
    finally:
        k1.close()
    paths, costs = host_gather(ctx, blocks)
    out.append(ctx.reduce_ragged(paths, costs, P))
    return out


def assert_all_equal(results, want_cost, want_path, want_log=None):
    for cost, log, path in results:
        assert cost.hex() == want_cost.hex()
        assert bits(path) == bits(want_path)
        if want_log is not None:
            assert log == want_log


# ---- 1. against the replay over the oracle's mergeBlocks -------------------------------------

CYCLE = [3 + b % 6 for b in range(12)]
REPLAY = [([3, 7, 4, 12, 5, 6, 3, 9], 1), ([3, 7, 4, 12, 5, 6, 3, 9], 2), ([3, 7, 4, 12, 5, 6, 3, 9], 3), (CYCLE, 8),
          ([20, 3, 20, 3], 1), ([9], 1)]


@pytest.mark.parametrize("ns,P", REPLAY, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else f"P{v}")
def test_ragged_forms_match_reference_replay(gpu_ctx, ns, P):
    blocks = ragged_blocks(ns, 1000 * len(ns) + P)
    sols = _solve_all(blocks)  # the oracle's per-block solutions
    want_path, want_cost = replay(sols, P)
    results = three_forms(gpu_ctx, blocks, P)
    assert_all_equal(results, want_cost, want_path, expected_log(ns, P))
    # and reduce_ragged on the oracle's own paths
    assert_all_equal([gpu_ctx.reduce_ragged([p for p, _ in sols], [c for _, c in sols], P)], want_cost, want_path,
                     expected_log(ns, P))


# ---- 2. stalls: near-ties resolved on the host, relaunches with the block's own length ---------

STALL_NS = [(4, 6, 9)[b % 3] for b in range(14)]


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("P", [1, 3])
def test_lattice_stalls_match_the_replay(gpu_ctx, knobs, P, persist):
    blocks = ragged_blocks(STALL_NS, 469 + P, kind="lattice")
    want_path, want_cost = replay(_solve_all(blocks), P)
    knobs.set("K3_PERSIST", persist)
    assert_all_equal(three_forms(gpu_ctx, blocks, P), want_cost, want_path, expected_log(STALL_NS, P))


# ---- 3. the LDS hand-over: the running path passes 4096 cities mid-rank -----------------------

CAP_NS = [(7, 8, 9)[b % 3] for b in range(520)]


@functools.lru_cache(maxsize=None)
def cap_case():
    blocks = ragged_blocks(CAP_NS, 520789)
    want_path, want_cost = replay(_solve_all(blocks), 1)
    assert len(want_path) > 4096
    return blocks, want_path, want_cost


@pytest.mark.parametrize("persist", [1, 0])
def test_path_outgrowing_the_lds_fold(gpu_ctx, knobs, persist):
    blocks, want_path, want_cost = cap_case()
    knobs.set("K3_PERSIST", persist)
    assert_all_equal(three_forms(gpu_ctx, blocks, 1), want_cost, want_path, "")


# ---- 4. the fold_ok decision -------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["dense", "equal", "spread", "two"])
def test_fold_decision_agrees_for_id_layouts(gpu_ctx, layout):
    """Dense ids take the one-kernel folds in both forms; equal ids force the
    general path in both; ids spread past the bitmap rule take it in the
    device form only; a 2-city block (an open path) forces it in both."""
    ns = [7, 4, 9, 5, 6, 3, 8, 7, 4, 9, 5, 6, 3, 8, 7, 4, 9, 5, 6, 3, 8, 7, 4, 9]
    P = 3
    if layout == "two":
        ns = [5, 2, 7]
        P = 1  # (the reference terminates for this one: checked by the replay below)
    blocks = ragged_blocks(ns, 7243)
    ident = {"dense": lambda b, i, g: g, "equal": lambda b, i, g: 5, "spread": lambda b, i, g: 10 ** 6 * b + i,
             "two": lambda b, i, g: g}[layout]
    blocks = [[(ident(b, i, cid), x, y) for i, (cid, x, y) in enumerate(blk)] for b, blk in enumerate(blocks)]
    paths, costs = host_gather(gpu_ctx, blocks)
    try:
        want = gpu_ctx.reduce_ragged(paths, costs, P)
        code = 0
    except tspgpu.TspGpuError as e:
        want, code = None, e.code
    k1 = RaggedK1(gpu_ctx, blocks)
    try:
        if code:
            with pytest.raises(tspgpu.TspGpuError) as e:
                k1.reduce(P)
            assert e.value.code == code
        else:
            cost, log, plen, path = k1.reduce(P)
            assert (cost.hex(), log, plen, bits(path)) == (want[0].hex(), want[1], len(want[2]), bits(want[2]))
    finally:
        k1.close()
    if layout == "two":
        assert code == 0
        want_path, want_cost = replay(_solve_all(blocks), P)
        assert_all_equal([want], want_cost, want_path)


# ---- 5. uniform input: every ragged entry returns what its uniform counterpart returns ---------

def uniform_equivalence(ctx, blocks, P):
    n, B = len(blocks[0]), len(blocks)
    # the pipelines
    want = ctx.pipeline_cities(blocks, P)
    got = ctx.pipeline_cities_ragged(blocks, P)
    assert (got[0].hex(), got[1], bits(got[2])) == (want[0].hex(), want[1], bits(want[2]))
    # the host fronts, on the same paths
    paths, costs = host_gather(ctx, blocks)
    want = ctx.reduce_path(paths, costs, P)
    got = ctx.reduce_ragged(paths, costs, P)
    assert (got[0].hex(), got[1], bits(got[2])) == (want[0].hex(), want[1], bits(want[2]))
    # the device fronts, each behind its own solve
    ku, kr = DeviceK1(ctx, blocks), RaggedK1(ctx, blocks, extra_stride=2)
    try:
        want, got = ku.reduce(P), kr.reduce(P)
        assert (got[0].hex(), got[1], got[2], bits(got[3])) == (want[0].hex(), want[1], want[2], bits(want[3]))
    finally:
        ku.close()
        kr.close()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_uniform_six_city_blocks_equal_the_uniform_forms(gpu_ctx, P):
    uniform_equivalence(gpu_ctx, make_blocks("random", 6, 4, 64 + P), P)


@pytest.mark.parametrize("B,P", TWO_CITY)
def test_two_city_blocks_equal_the_uniform_forms(gpu_ctx, B, P):
    uniform_equivalence(gpu_ctx, two_city_blocks(B), P)


# ---- 6. errors -------------------------------------------------------------------------------

ERR_NS = [6, 4, 9, 5, 7, 3, 8]


@pytest.mark.parametrize("where", [0, 3, 6])
def test_bad_status_fails_before_anything_is_merged(gpu_ctx, where):
    """A NaN coordinate fails its own block in K1 (status -EINVAL, row -1); the
    reduce then fails with that code and leaves d_path_out alone."""
    blocks = ragged_blocks(ERR_NS, 69)
    cid, x, y = blocks[where][1]
    blocks[where][1] = (cid, float("nan"), y)
    k1 = RaggedK1(gpu_ctx, blocks)
    try:
        gpu_ctx.synchronize(0)  # (the solve was left running on the stream it was given)
        status = gpu_ctx.download(k1.status, (k1.B,), np.int32)
        assert status.tolist() == [EINVAL if b == where else 0 for b in range(k1.B)]
        d_path = k1.path_buffer(64, fill=(-7, -7.0, -7.0))
        with pytest.raises(tspgpu.TspGpuError) as e:
            k1.reduce(1, cap=64, d_path=d_path)
        assert e.value.code == EINVAL
        assert k1.download_path(d_path, 64) == [(-7, -7.0, -7.0)] * 64
    finally:
        k1.close()
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.pipeline_cities_ragged(blocks, 1)
    assert e.value.code == EINVAL


@pytest.mark.parametrize("entry", ["n", "-1"])
def test_tour_entry_out_of_range_is_refused(gpu_ctx, entry):
    """Block 1 (4 cities) shares its wave with blocks 0 and 2: an entry of
    n_b = 4, in range for both neighbours, and one of -1, under status 0."""
    blocks = ragged_blocks(ERR_NS, 69)
    k1 = RaggedK1(gpu_ctx, blocks)
    try:
        gpu_ctx.synchronize(0)  # (the solve was left running on the stream it was given: it writes the rows poked below)
        tour = gpu_ctx.download(k1.tour, (k1.B, k1.stride), np.int32)
        tour[1, 2] = 4 if entry == "n" else -1
        k1.poke(k1.tour, tour)
        with pytest.raises(tspgpu.TspGpuError) as e:
            k1.reduce(1)
        assert e.value.code == EINVAL
    finally:
        k1.close()
    a, b = gpu_ctx.pipeline_cities_ragged(blocks, 1), gpu_ctx.pipeline_cities_ragged(blocks, 1)
    assert (a[0].hex(), a[1], bits(a[2])) == (b[0].hex(), b[1], bits(b[2]))  # the context goes on working


def test_short_capacity_and_length_query(gpu_ctx):
    blocks = ragged_blocks(ERR_NS, 69)
    paths, costs = host_gather(gpu_ctx, blocks)
    hcost, hlog, hpath = gpu_ctx.reduce_ragged(paths, costs, 2)
    full = len(hpath)
    for cap in (full - 1, 0):
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.reduce_ragged(paths, costs, 2, path_cap=cap)
        assert e.value.code == ENOSPC and e.value.path_len == full
        assert (e.value.cost, e.value.log) == (hcost, hlog)
        assert bits(e.value.path) == bits(hpath[:cap])
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.pipeline_cities_ragged(blocks, 2, path_cap=cap)
        assert e.value.code == ENOSPC and e.value.path_len == full and (e.value.cost, e.value.log) == (hcost, hlog)
        assert bits(e.value.path) == bits(hpath[:cap])
    k1 = RaggedK1(gpu_ctx, blocks)
    try:
        d_path = k1.path_buffer(full, fill=(-7, -7.0, -7.0))
        with pytest.raises(tspgpu.TspGpuError) as e:
            k1.reduce(2, cap=full - 1, d_path=d_path)
        assert e.value.code == ENOSPC and e.value.path_len == full
        assert (e.value.cost, e.value.log) == (hcost, hlog)
        got = k1.download_path(d_path, full)
        assert bits(got[:full - 1]) == bits(hpath[:full - 1]) and got[full - 1] == (-7, -7.0, -7.0)
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.reduce_ragged_device(k1.cities, k1.ns, k1.tour, k1.stride, k1.cost, k1.status, 2)  # NULL, 0
        assert e.value.code == ENOSPC and e.value.path_len == full and e.value.cost == hcost
    finally:
        k1.close()


# ---- 7. a caller stream ---------------------------------------------------------------------

def test_caller_stream(gpu_ctx):
    ns = [3 + (5 * b) % 14 for b in range(60)]
    blocks = ragged_blocks(ns, 9120)
    k0 = RaggedK1(gpu_ctx, blocks)
    st = gpu_ctx.stream_create()
    k1 = None
    try:
        base = k0.reduce(4)
        k1 = RaggedK1(gpu_ctx, blocks, stream=st)  # K1's outputs produced on st, not waited for
        got = k1.reduce(4, stream=st)
        assert (got[0].hex(), got[1], got[2], bits(got[3])) == (base[0].hex(), base[1], base[2], bits(base[3]))
    finally:
        gpu_ctx.synchronize(st)
        k0.close()
        if k1:
            k1.close()
        gpu_ctx.stream_destroy(st)
