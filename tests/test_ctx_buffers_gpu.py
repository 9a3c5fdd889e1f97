"""The context's buffers across calls, streams and destruction (csrc/ctx.h over
csrc/hipbuf.h): grow-only reserves that keep the larger buffer, the pinned
descriptor uploads when calls on two streams follow each other without a
synchronisation, a stream destroyed behind a pending upload, and every owner
of the context reached before it is released.

Nothing here has a tolerance: every answer is compared bit for bit (costs as
uint64, tours entry by entry, rows padded with -1) with the same blocks solved
one size at a time through solve_blocks on the session's context.  Cities are
the reference generator's, renumbered so that ids are unique across blocks."""
import numpy as np
import pytest

import tspgpu
from test_cities_device_gpu import _carray
from test_cities_ragged_gpu import host_dist, packed, ragged_cities

pytestmark = pytest.mark.gpu

U64 = np.uint64
_REF = {}


def make_blocks(sizes, seed):
    blocks = ragged_cities(list(sizes), seed)
    at = 0
    for blk in blocks:
        blk["id"] = np.arange(at, at + len(blk))
        at += len(blk)
    return blocks


def reference(ref_ctx, sizes, seed):
    """-> (blocks, cost (B,), tours: list of lists): solve_blocks on the blocks of each size, computed once."""
    key = (tuple(sizes), seed)
    if key not in _REF:
        blocks = make_blocks(sizes, seed)
        cost, tours = np.zeros(len(blocks)), [None] * len(blocks)
        for n in sorted(set(sizes)):
            idx = [b for b, k in enumerate(sizes) if k == n]
            c, t = ref_ctx.solve_blocks(np.stack([host_dist(blocks[b]) for b in idx]))
            for j, b in enumerate(idx):
                cost[b], tours[b] = c[j], t[j][: tspgpu.tour_length(n)].tolist()
        _REF[key] = (blocks, cost, tours)
    return _REF[key]


def assert_same(ref, cost, tour, status=None):
    blocks, rcost, rtours = ref
    assert np.array_equal(np.asarray(cost, np.float64).view(U64), rcost.view(U64))
    for b, rt in enumerate(rtours):
        assert tour[b][: len(rt)].tolist() == rt and (tour[b][len(rt):] == -1).all(), (b, tour[b].tolist())
    assert status is None or not np.asarray(status).any()


def sizes_of(B, lo, hi):
    return [lo + b % (hi - lo + 1) for b in range(B)]


def tuples(blk):
    return [(int(c["id"]), float(c["x"]), float(c["y"])) for c in blk]


# the four host forms: (sizes of a batch of B, the call on (ctx, blocks) -> (cost, tour, status or None))
FORMS = {
    "solve_blocks": (lambda B: [7] * B,
                     lambda ctx, bl: ctx.solve_blocks(np.stack([host_dist(b) for b in bl])) + (None,)),
    "solve_ragged": (lambda B: sizes_of(B, 5, 8), lambda ctx, bl: ctx.solve_ragged([host_dist(b) for b in bl])),
    "solve_cities_ragged": (lambda B: sizes_of(B, 5, 8),
                            lambda ctx, bl: ctx.solve_cities_ragged((_carray(packed(bl)), [len(b) for b in bl]))),
    "solve_cities_upload": (lambda B: [7] * B,
                            lambda ctx, bl: ctx.solve_cities((_carray(packed(bl)), 7, len(bl)), device_dist=True)
                            + (None,)),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_grow_shrink_grow_on_one_context(gpu_ctx, form):
    """4 blocks, then 300, then 4 (other blocks) on one context, nothing destroyed in between: the reserves keep the
    larger buffers and the round trip copies the sizes of each call."""
    sizes, call = FORMS[form]
    with tspgpu.Context(device=0) as ctx:
        for seed, B in enumerate((4, 300, 4)):
            ref = reference(gpu_ctx, sizes(B), seed)
            assert_same(ref, *call(ctx, ref[0]))


class DeviceRagged:
    """The device arrays of one solve_ragged_device / solve_cities_ragged_device call."""

    def __init__(self, ctx, blocks, cities=False):
        self.ctx, self.ns, self.B = ctx, [len(b) for b in blocks], len(blocks)
        self.stride = max(self.ns) + 1
        sq = np.array([n * n for n in self.ns], np.int64)
        self.offset = np.concatenate(([0], np.cumsum(sq)[:-1]))
        src = packed(blocks).view(np.uint8) if cities else np.concatenate([host_dist(b).ravel() for b in blocks])
        self.d_in = ctx.upload(src)
        self.d_cost = ctx.upload(np.full(self.B, 7.0))
        self.d_tour = ctx.upload(np.full(self.B * self.stride, 7, np.int32))
        self.d_status = ctx.upload(np.full(self.B, 7, np.int32))

    def results(self):
        c = self.ctx
        return (c.download(self.d_cost, (self.B,), np.float64), c.download(self.d_tour, (self.B, self.stride), np.int32),
                c.download(self.d_status, (self.B,), np.int32))

    def free(self):
        for p in (self.d_in, self.d_cost, self.d_tour, self.d_status):
            self.ctx.free(p)


def test_descriptor_reuse_across_streams(gpu_ctx):
    """Two ragged calls back to back, no synchronisation between them: 8 blocks on a created stream, then 200 on the
    context's stream (the pinned descriptor buffer grows while the first upload may be pending), then a ragged
    distance build on the created stream."""
    ref_a, ref_b = reference(gpu_ctx, sizes_of(8, 5, 9), 3), reference(gpu_ctx, sizes_of(200, 5, 9), 4)
    blocks_c = make_blocks(sizes_of(8, 5, 9), 5)
    with tspgpu.Context(device=0) as ctx:
        a, b = DeviceRagged(ctx, ref_a[0]), DeviceRagged(ctx, ref_b[0])
        ns_c = [len(blk) for blk in blocks_c]
        elems = sum(n * n for n in ns_c)
        d_cc, d_cd = ctx.upload(packed(blocks_c).view(np.uint8)), ctx.upload(np.full(elems, -7.0))
        s1 = ctx.stream_create()
        try:
            ctx.solve_ragged_device(a.d_in, tspgpu.F64, a.offset, a.ns, a.d_cost, a.d_tour, a.stride, a.d_status, s1)
            ctx.solve_ragged_device(b.d_in, tspgpu.F64, b.offset, b.ns, b.d_cost, b.d_tour, b.stride, b.d_status,
                                    ctx.stream)
            ctx.distance_matrix_ragged_device(d_cc, ns_c, d_cd, s1)
            ctx.synchronize(s1)
            ctx.synchronize()
            assert_same(ref_a, *a.results())
            assert_same(ref_b, *b.results())
            flat, at = ctx.download(d_cd, (elems,), np.float64), 0
            for blk in blocks_c:
                n = len(blk)
                assert np.array_equal(flat[at:at + n * n].view(U64), host_dist(blk).ravel().view(U64))
                at += n * n
        finally:
            ctx.synchronize(s1)
            ctx.stream_destroy(s1)
            a.free(), b.free(), ctx.free(d_cc), ctx.free(d_cd)


def test_stream_destroy_drains_the_pending_uploads(gpu_ctx):
    """solve_cities_ragged_device on a created stream, the stream destroyed at once, the same call on the context's
    stream: both outputs, read after a synchronisation, are right."""
    ref = reference(gpu_ctx, sizes_of(12, 5, 9), 6)
    with tspgpu.Context(device=0) as ctx:
        a, b = DeviceRagged(ctx, ref[0], cities=True), DeviceRagged(ctx, ref[0], cities=True)
        try:
            s1 = ctx.stream_create()
            ctx.solve_cities_ragged_device(a.d_in, a.ns, a.d_cost, a.d_tour, a.stride, a.d_status, s1)
            ctx.stream_destroy(s1)
            ctx.solve_cities_ragged_device(b.d_in, b.ns, b.d_cost, b.d_tour, b.stride, b.d_status, ctx.stream)
            ctx.synchronize()
            assert_same(ref, *a.results())
            assert_same(ref, *b.results())
        finally:
            a.free(), b.free()


def test_mixed_fronts_then_destroy_twice(gpu_ctx):
    """One call of every front on a fresh context, then ctx_destroy; a second context repeats it: the same answers
    both times, each the reference's.  Reaches every owner of the context before its release."""
    ragged, uniform = reference(gpu_ctx, [5, 6, 7, 8, 5, 6], 7), reference(gpu_ctx, [7] * 6, 8)
    d18, d10 = (host_dist(blk) for blk in make_blocks([18, 10], 9))
    want18, want10 = gpu_ctx.solve_blocks(d18[None]), gpu_ctx.solve_blocks(d10[None])
    upaths = [[tuples(blk)[t] for t in tour] for blk, tour in zip(uniform[0], uniform[2])]
    rpaths = [[tuples(blk)[t] for t in tour] for blk, tour in zip(ragged[0], ragged[2])]
    want_pipe, want_rpipe = gpu_ctx.reduce_path(upaths, uniform[1], 2), gpu_ctx.reduce_ragged(rpaths, ragged[1], 2)
    answers = []
    for _ in range(2):
        ctx = tspgpu.Context(device=0)
        try:
            assert_same(ragged, *ctx.solve_ragged([host_dist(b) for b in ragged[0]]))
            assert_same(uniform, *ctx.solve_cities((_carray(packed(uniform[0])), 7, 6), device_dist=True))
            assert_same(ragged, *ctx.solve_cities_ragged((_carray(packed(ragged[0])), [len(b) for b in ragged[0]])))
            pipe = ctx.pipeline_cities([tuples(b) for b in uniform[0]], 2)
            rpipe = ctx.pipeline_cities_ragged([tuples(b) for b in ragged[0]], 2)
            assert pipe == want_pipe and rpipe == want_rpipe
            c18, t18, _ = ctx.solve_instance(d18)
            assert c18 == want18[0][0] and t18.tolist() == want18[1][0].tolist()
            c10, t10, _ = tspgpu.search_solve(ctx, d10)
            assert c10 == want10[0][0] and list(t10) == want10[1][0].tolist()
            answers.append((pipe, rpipe, c18, t18.tolist(), c10, list(t10)))
        finally:
            ctx.close()
    assert answers[0] == answers[1]
