"""K1's device results reduced in place, and the merged tour (csrc/paths.hip,
the core of csrc/merge.hip): tspgpu_reduce_path against a
Python replay of the reference's schedule over the oracle's mergeBlocks, the
device form (tspgpu_reduce_device behind tspgpu_solve_cities_device) against
the host form bit for bit, the fold_ok decision under three id layouts, the
error contract, a caller stream, and tspgpu_pipeline_cities against the
reference's own output (tests/golden/cli.json)."""
import ctypes
import errno
import math
import re

import numpy as np
import pytest

import oracle_py as O
import tspgpu
from test_host import H, _solve_all, generate

pytestmark = pytest.mark.gpu
FINAL = re.compile(r"trip cost (\S+)$")


def bits(path):
    """(id, x, y) with the coordinates' bit patterns: equality is bitwise."""
    return [(int(c[0]), float(c[1]).hex(), float(c[2]).hex()) for c in path]


def replay(sols, P):
    """The reference's schedule (tsp.cpp:52-134, 167-192, 348-352) over the
    oracle's mergeBlocks: distribution counts, every rank's left fold, the
    receives with their stale function-local lists -> (rank 0's path, cost)."""
    B = len(sols)
    cnt = [0] * P
    for b in range(1, B + 1):
        cnt[b % P] += 1
    rank, rcost, nxt = [], [], 0
    for r in range(P):
        path, cost = sols[nxt]
        nxt += 1
        for _ in range(1, cnt[r]):
            path, cost = O.merge_blocks(path, cost, *sols[nxt])
            nxt += 1
        rank.append(list(path))
        rcost.append(cost)
    acc = [[] for _ in range(P)]

    def receive(to, frm):
        acc[to] = acc[to] + rank[frm]
        rank[to], rcost[to] = O.merge_blocks(rank[to], rcost[to], acc[to], rcost[frm])

    lastpower = 1 << int(math.log2(P))
    for i in range(P - lastpower):
        receive(i, i + lastpower)
    d = 0
    while (1 << d) < lastpower:
        for k in range(0, lastpower, 1 << (d + 1)):
            receive(k, k + (1 << d))
        d += 1
    return rank[0], rcost[0]


def host_reduce_rc(sols, P):
    """tsphost_reduce's return code (0: the reference terminates) and cost."""
    B, L = len(sols), len(sols[0][0])
    flat = (tspgpu.City * (B * L))()
    costs = (ctypes.c_double * B)()
    for b, (path, cost) in enumerate(sols):
        costs[b] = cost
        for i, (cid, x, y) in enumerate(path):
            flat[b * L + i].id, flat[b * L + i].x, flat[b * L + i].y = cid, x, y
    final = ctypes.c_double()
    rc = H.tsphost_reduce(flat, L, costs, B, P, ctypes.byref(final), None, 0)
    return rc, final.value


def make_blocks(kind, n, B, seed):
    """The blocks of tests/test_merge_gpu.py::test_persistent_fold_matches_host."""
    rng = np.random.default_rng(seed)
    blocks = []
    for b in range(B):
        xy = (rng.integers(0, 3, size=(n, 2)) + 3 * np.array([b % 7, b // 7])).astype(np.float64) \
            if kind == "lattice" else rng.uniform(0, 1000, size=(n, 2))
        blocks.append([(b * n + i, xy[i, 0], xy[i, 1]) for i in range(n)])
    return blocks


# ---- 1. the final path against the reference's merge -------------------------------

REPLAY = [(6, 4, 1), (6, 4, 2), (6, 4, 3), (12, 4, 4), (5, 12, 8), (3, 2, 1), (6, 4, 4), (6, 1, 1)]


@pytest.mark.parametrize("n,B,P", REPLAY, ids=lambda v: str(v))
def test_reduce_path_matches_reference_replay(gpu_ctx, n, B, P):
    sols = _solve_all(generate(n, B, 1000, 1000))
    want_path, want_cost = replay(sols, P)
    paths, costs = [p for p, _ in sols], [c for _, c in sols]
    cost, log, path = gpu_ctx.reduce_path(paths, costs, P)
    assert cost.hex() == want_cost.hex()
    assert bits(path) == bits(want_path)
    assert (cost, log) == gpu_ctx.reduce(paths, costs, P)


# ---- 2. the device form equals the host form, bitwise -----------------------------


class DeviceK1:
    """Cities uploaded and solved on the device (tspgpu_solve_cities_device):
    the pointers tspgpu_reduce_device takes."""

    def __init__(self, ctx, blocks, stream=0):
        self.ctx = ctx
        arr, self.n, self.B = tspgpu.cities_array(blocks)
        n, B = self.n, self.B
        self.L = tspgpu.tour_length(n)
        self.ptrs = []
        self.cities = self._keep(ctx.upload(np.frombuffer(arr, dtype=tspgpu.CITY_DTYPE, count=B * n)))
        self.cost = self._keep(ctx.alloc(8 * B))
        self.tour = self._keep(ctx.alloc(4 * B * (n + 1)))
        self.status = self._keep(ctx.alloc(4 * B))
        ctx.solve_cities_device(self.cities, n, B, self.cost, self.tour, self.status, stream)
        self.k1_stream = stream

    def _keep(self, p):
        self.ptrs.append(p)
        return p

    def path_buffer(self, cap, fill=None):
        init = np.zeros(max(cap, 1), dtype=tspgpu.CITY_DTYPE)
        if fill is not None:
            init["id"], init["x"], init["y"] = fill
        return self._keep(self.ctx.upload(init))

    def reduce(self, P, cap=None, stream=0, status=True, d_path=None):
        """-> (cost, log, path length, downloaded path as (id, x, y) tuples)"""
        if cap is None:
            cap = 6 * self.B * self.L + 1  # (stale lists: below 13/8 of the cities at P = 8)
        if d_path is None:
            d_path = self.path_buffer(cap)
        cost, log, plen = self.ctx.reduce_device(self.cities, self.tour, self.cost, self.status if status else 0,
                                                 self.n, self.B, P, d_path, cap, stream)
        return cost, log, plen, self.download_path(d_path, plen)

    def download_path(self, d_path, count):
        got = self.ctx.download(d_path, (count,), tspgpu.CITY_DTYPE)
        return [(int(c["id"]), float(c["x"]), float(c["y"])) for c in got]

    def poke(self, ptr, arr):
        # (K1 is left running on its stream, and the copy below goes through the
        # context's: without this wait K1's scatter can overwrite what is poked)
        self.ctx.synchronize(self.k1_stream)
        arr = np.ascontiguousarray(arr)
        rc = tspgpu.lib().tspgpu_memcpy_htod(self.ctx.handle, ptr, arr.ctypes.data, arr.nbytes)
        assert rc == 0

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


def host_form(ctx, blocks, P):
    """solve_cities, the host gather (convPathToCityPath), reduce_path"""
    cost, tour = ctx.solve_cities(blocks)
    L = tspgpu.tour_length(len(blocks[0]))
    paths = [[blk[t] for t in tour[b][:L]] for b, blk in enumerate(blocks)]
    return ctx.reduce_path(paths, cost, P)


def assert_forms_agree(ctx, blocks, P, **kw):
    hcost, hlog, hpath = host_form(ctx, blocks, P)
    k1 = DeviceK1(ctx, blocks)
    try:
        dcost, dlog, dlen, dpath = k1.reduce(P, **kw)
    finally:
        k1.close()
    assert dcost.hex() == hcost.hex()
    assert dlog == hlog
    assert dlen == len(hpath)
    assert bits(dpath) == bits(hpath)
    return hcost, hlog, hpath


FOLD_SHAPES = [("lattice", 6, 48, 1), ("lattice", 9, 40, 3), ("random", 8, 300, 8), ("random", 5, 1100, 1)]


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("kind,n,B,P", FOLD_SHAPES)
def test_device_form_equals_host_form(gpu_ctx, knobs, kind, n, B, P, persist):
    """Near-tie stalls resolved on the host, eight ranks, a path outgrowing the
    4096-city LDS fold; the persistent fold and the per-merge kernels."""
    knobs.set("K3_PERSIST", persist)
    assert_forms_agree(gpu_ctx, make_blocks(kind, n, B, n * 1000 + B + P), P)


def test_device_form_equals_host_form_16_cities(gpu_ctx):
    assert_forms_agree(gpu_ctx, make_blocks("random", 16, 64, 16064), 1)


# n = 2 blocks (tour rows [1, 0]: two cities, no closing copy) with the (B, P)
# the reference terminates for (tests/test_pipeline_abi.py checks that premise
# on the CPU: most other (B, P) loop forever in its mergeBlocks)
TWO_CITY = [(2, 1), (2, 2), (3, 3), (5, 2)]


def two_city_blocks(B):
    return make_blocks("random", 2, B, 22)


@pytest.mark.parametrize("B,P", TWO_CITY)
def test_device_form_equals_host_form_two_cities(gpu_ctx, B, P):
    _, _, path = assert_forms_agree(gpu_ctx, two_city_blocks(B), P)
    if P == 1:
        assert len(path) == 2 + (B - 1)  # (each merge adds L - 1 = 1 city)


def test_device_form_equals_host_form_three_cities(gpu_ctx):
    assert_forms_agree(gpu_ctx, make_blocks("random", 3, 37, 337), 2)
    # without statuses (the caller's guarantee) the answer is the same
    assert_forms_agree(gpu_ctx, make_blocks("random", 3, 37, 337), 2, status=False)


# ---- 3. the fold_ok decision -----------------------------------------------------


@pytest.mark.parametrize("layout", ["dense", "equal", "spread"])
def test_fold_decision_agrees_for_id_layouts(gpu_ctx, layout):
    """Dense ids take the one-kernel folds in both forms; equal ids force the
    general path in both; ids spread past the bitmap rule take it in the
    device form only, and must give the same answer."""
    n, B, P = 7, 24, 3
    blocks = make_blocks("random", n, B, 7243)
    ident = {"dense": lambda b, i: b * n + i, "equal": lambda b, i: 5, "spread": lambda b, i: 10 ** 6 * b + i}[layout]
    blocks = [[(ident(b, i), x, y) for i, (_, x, y) in enumerate(blk)] for b, blk in enumerate(blocks)]
    assert_forms_agree(gpu_ctx, blocks, P)


def test_id_range_ending_in_the_bitmaps_last_partial_word(gpu_ctx):
    """B * L = 15 is no multiple of 4 and the ids span 8 * B * L - 1: the
    widest range the bitmap rule accepts, whose last bit lies in the bitmap's
    last, partial 32-bit word (the bitmap is allocated in whole words)."""
    n, B = 4, 3
    L = tspgpu.tour_length(n)
    blocks = make_blocks("random", n, B, 4315)
    last = 8 * B * L - 1 - 7
    blocks = [[(last if (b, i) == (B - 1, n - 1) else b * n + i - 7, x, y) for i, (_, x, y) in enumerate(blk)]
              for b, blk in enumerate(blocks)]
    assert_forms_agree(gpu_ctx, blocks, 1)


# ---- 4. errors ----------------------------------------------------------------


def test_pipeline_rejects_nan_and_context_survives(gpu_ctx):
    blocks = make_blocks("random", 6, 9, 69)
    bad = [list(b) for b in blocks]
    bad[4][2] = (bad[4][2][0], float("nan"), bad[4][2][2])
    with pytest.raises(tspgpu.TspGpuError) as e:
        gpu_ctx.pipeline_cities(bad, 2)
    assert e.value.code == -errno.EINVAL
    cost, log, path = gpu_ctx.pipeline_cities(blocks, 2)
    assert (cost, log, bits(path)) == (lambda r: (r[0], r[1], bits(r[2])))(host_form(gpu_ctx, blocks, 2))


def test_bad_status_fails_before_anything_is_merged(gpu_ctx):
    blocks = make_blocks("random", 6, 9, 69)
    k1 = DeviceK1(gpu_ctx, blocks)
    try:
        status = np.zeros(9, dtype=np.int32)
        status[3], status[6] = -errno.ERANGE, -errno.EINVAL
        k1.poke(k1.status, status)
        # (the rows of bad blocks hold -1, as K1 leaves them.  The return code
        # cannot show whether the kernel read them: the status wins either way.
        # That such a row is skipped is checked on the serial twin of the
        # kernel, host/check_paths.cpp.)
        tour = gpu_ctx.download(k1.tour, (9, 7), np.int32)
        tour[3, :] = -1
        tour[6, :] = -1
        k1.poke(k1.tour, tour)
        d_path = k1.path_buffer(64, fill=(-7, -7.0, -7.0))
        with pytest.raises(tspgpu.TspGpuError) as e:
            k1.reduce(1, cap=64, d_path=d_path)
        assert e.value.code == -errno.ERANGE  # the first such block's code
        assert k1.download_path(d_path, 64) == [(-7, -7.0, -7.0)] * 64
    finally:
        k1.close()


@pytest.mark.parametrize("entry", ["n", "-1"])
def test_tour_entry_out_of_range_is_refused(gpu_ctx, entry):
    """The kernel checks an entry before it indexes with it: -EINVAL, and the
    context goes on working."""
    blocks = make_blocks("random", 6, 9, 69)
    k1 = DeviceK1(gpu_ctx, blocks)
    try:
        tour = gpu_ctx.download(k1.tour, (9, 7), np.int32)
        tour[5, 3] = 6 if entry == "n" else -1
        k1.poke(k1.tour, tour)
        with pytest.raises(tspgpu.TspGpuError) as e:
            k1.reduce(1)
        assert e.value.code == -errno.EINVAL
    finally:
        k1.close()
    assert_forms_agree(gpu_ctx, blocks, 1)


def test_short_capacity_and_length_query(gpu_ctx):
    blocks = make_blocks("random", 6, 9, 69)
    hcost, hlog, hpath = host_form(gpu_ctx, blocks, 2)
    full = len(hpath)
    cost, tour = gpu_ctx.solve_cities(blocks)
    paths = [[blk[t] for t in tour[b]] for b, blk in enumerate(blocks)]
    # host form: one short, and the length query with NULL
    for cap in (full - 1, 0):
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.reduce_path(paths, cost, 2, path_cap=cap)
        assert e.value.code == -errno.ENOSPC and e.value.path_len == full
        assert (e.value.cost, e.value.log) == (hcost, hlog)
        assert bits(e.value.path) == bits(hpath[:cap])
    # device form
    k1 = DeviceK1(gpu_ctx, blocks)
    try:
        d_path = k1.path_buffer(full, fill=(-7, -7.0, -7.0))
        with pytest.raises(tspgpu.TspGpuError) as e:
            k1.reduce(2, cap=full - 1, d_path=d_path)
        assert e.value.code == -errno.ENOSPC and e.value.path_len == full
        assert (e.value.cost, e.value.log) == (hcost, hlog)
        got = k1.download_path(d_path, full)
        assert bits(got[:full - 1]) == bits(hpath[:full - 1]) and got[full - 1] == (-7, -7.0, -7.0)
        with pytest.raises(tspgpu.TspGpuError) as e:
            gpu_ctx.reduce_device(k1.cities, k1.tour, k1.cost, k1.status, k1.n, k1.B, 2)  # NULL, 0
        assert e.value.code == -errno.ENOSPC and e.value.path_len == full and e.value.cost == hcost
    finally:
        k1.close()


# ---- 5. a caller stream ---------------------------------------------------------


def test_caller_stream(gpu_ctx):
    blocks = make_blocks("random", 9, 120, 9120)
    k0 = DeviceK1(gpu_ctx, blocks)
    st = gpu_ctx.stream_create()
    k1 = None
    try:
        base = k0.reduce(4)
        k1 = DeviceK1(gpu_ctx, blocks, stream=st)  # K1's outputs produced on st, not waited for
        got = k1.reduce(4, stream=st)
        assert (got[0].hex(), got[1], got[2], bits(got[3])) == (base[0].hex(), base[1], base[2], bits(base[3]))
    finally:
        gpu_ctx.synchronize(st)
        k0.close()
        if k1:
            k1.close()
        gpu_ctx.stream_destroy(st)


# ---- 6. pipeline_cities against the reference's output ------------------------------

CLI = [c for c in O.load_golden("cli.json") if not c.get("error_case") and c["args"][0] >= 3]


@pytest.mark.parametrize("case", CLI, ids=lambda c: "-".join(map(str, c["args"])) + f"-P{c['P']}")
def test_pipeline_matches_mpirun(gpu_ctx, case):
    n, B, X, Y = case["args"]
    final, log, path = gpu_ctx.pipeline_cities(generate(n, B, X, Y), case["P"])
    assert "%f" % final == FINAL.search(case["lines"][-1]).group(1)
    assert sorted(log.splitlines()) == sorted(ln for ln in case["lines"] if ln.startswith("process "))
    if case["P"] == 1:  # a closed tour over every city
        assert path[0] == path[-1] and sorted(c[0] for c in path[:-1]) == list(range(n * B))
