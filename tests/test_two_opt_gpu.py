"""2-opt with a neighbour grid on the GPU (tspgpu_two_opt_path*)
against the Python model of its contract (tests/two_opt_model.py).

Nothing here has a tolerance: the path is compared id by id and coordinate
bit by coordinate bit, passes, candidates and moves exactly, `gain` as bits.
tests/test_two_opt_model.py shows that every input here (but the ones made to
move nothing) has moves applied in the model, so these are not comparisons of
untouched paths."""
import ctypes
import errno
import math
import struct

import numpy as np
import pytest

import oracle_py as O
import refine_model as R
import tspgpu
import two_opt_model as T

pytestmark = pytest.mark.gpu

KEYS = ("passes", "candidates", "moves")


def bits(v):
    return struct.pack("<d", v)


def same_path(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and bits(x[1]) == bits(y[1]) and bits(x[2]) == bits(y[2])
                                    for x, y in zip(a, b))


def same_stats(got, want):
    return all(got[k] == want[k] for k in KEYS) and bits(got["gain"]) == bits(want["gain"])


def check_model(ctx, name):
    path, ring, passes, want, wstats = T.solved(name)
    got, stats = ctx.two_opt_path(list(path), ring, passes)
    assert same_stats(stats, wstats), (stats, wstats)
    assert same_path(got, want)
    return path, got, stats


@pytest.mark.parametrize("name", sorted(T.IDLE_INPUTS))
def test_nothing_to_do_matches_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert same_path(got, path) and stats["moves"] == 0


@pytest.mark.parametrize("name", sorted(T.MOVING_INPUTS))
def test_inputs_match_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert stats["moves"] >= 1 and tspgpu.path_length(got) < tspgpu.path_length(path)
    assert sorted(got) == sorted(path) and got[0] == path[0] and got[-1] == path[-1]


@pytest.mark.parametrize("name", sorted(T.CUT_INPUTS))
def test_runs_cut_by_max_passes_match_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert stats["passes"] == T.built(name)[2] and stats["moves"] >= 1


def on_device(ctx, path, ring, passes):
    """The device form on an upload of `path` -> (rc or stats, the path after)."""
    arr, L, _ = tspgpu.cities_array([path])
    d_path = ctx.upload(np.frombuffer(arr, np.uint8))
    try:
        try:
            out = ctx.two_opt_path_device(d_path, L, ring, passes, ctx.stream)
        except tspgpu.TspGpuError as err:
            out = err.code
        raw = ctx.download(d_path, (L,), tspgpu.CITY_DTYPE)
    finally:
        ctx.free(d_path)
    return out, [(int(c["id"]), float(c["x"]), float(c["y"])) for c in raw]


@pytest.mark.parametrize("name", ["scrambled-400", "reversed-sweep-2000", "L3", "bow-tie"])
def test_host_form_equals_device_form(gpu_ctx, name):
    path, ring, passes, want, wstats = T.solved(name)
    stats, got = on_device(gpu_ctx, path, ring, passes)
    assert same_stats(stats, wstats) and same_path(got, want)


def test_refused_paths_return_the_codes_and_stay(gpu_ctx):
    base = list(T.built("scrambled-400")[0])
    cases = []
    for bad in (math.nan, math.inf, -math.inf):
        for at, axis in ((0, 1), (137, 2), (399, 1)):
            path = [list(c) for c in base]
            path[at][axis] = bad
            cases.append(([tuple(c) for c in path], -errno.EINVAL))
    wide = list(base)
    wide[5] = (wide[5][0], -1.0e308, wide[5][2])
    wide[300] = (wide[300][0], 1.0e308, wide[300][2])
    cases.append((wide, -errno.ERANGE))
    square = list(base)  # both extents finite, the sum of their squares not
    square[9] = (square[9][0], 1.0e200, square[9][2])
    cases.append((square, -errno.ERANGE))
    cases.append(([(0, math.nan, 1.0), (1, 2.0, 3.0)], -errno.EINVAL))  # validated also where nothing could move
    for path, code in cases:
        assert T.two_opt(path)[1] == code
        rc, after = on_device(gpu_ctx, path, 2, 1000)
        assert rc == code
        assert all(a[0] == b[0] and bits(a[1]) == bits(b[1]) and bits(a[2]) == bits(b[2]) for a, b in zip(after, path))
        # the host form writes neither the output nor the stats
        arr, L, _ = tspgpu.cities_array([path])
        out = (tspgpu.City * L)()
        st = tspgpu.TwoOptStats(passes=7)
        assert tspgpu.lib().tspgpu_two_opt_path(gpu_ctx.handle, arr, L, 2, 1000, out, ctypes.byref(st)) == code
        assert st.passes == 7 and all(c.id == 0 and c.x == 0.0 for c in out)
    # the context still works
    check_model(gpu_ctx, "scrambled-400-cut3")


def test_bad_arguments_on_a_live_context(gpu_ctx):
    path = list(T.built("bow-tie")[0])
    for ring, passes in ((0, 8), (5, 8), (2, 0), (-1, 8)):
        with pytest.raises(tspgpu.TspGpuError) as err:
            gpu_ctx.two_opt_path(path, ring, passes)
        assert err.value.code == -errno.EINVAL


def test_in_place_host_form(gpu_ctx):
    path, ring, passes, want, wstats = T.solved("closed-tour-251")
    arr, L, _ = tspgpu.cities_array([path])
    st = tspgpu.TwoOptStats()
    assert tspgpu.lib().tspgpu_two_opt_path(gpu_ctx.handle, arr, L, ring, passes, arr, ctypes.byref(st)) == 0
    assert same_stats(st.as_dict(), wstats) and same_path([(arr[i].id, arr[i].x, arr[i].y) for i in range(L)], want)
    assert tspgpu.lib().tspgpu_two_opt_path(gpu_ctx.handle, arr, L, ring, passes, arr, None) == 0  # stats may be NULL


def test_pipeline_keywords_are_the_separate_calls(gpu_ctx):
    blocks = O.generate(8, 64, 1000, 1000)
    final, log, tour = gpu_ctx.pipeline_cities(blocks, 1)
    # (the model's shared run of this case starts from the oracle's merge of the same batch)
    shared, ring, passes, want, wstats = T.solved("generator-8x64")
    if not same_path(tour, shared):
        want, wstats = T.two_opt(tour, ring, passes)
    tpath, tstats = gpu_ctx.two_opt_path(tour, 2, 1000)
    assert same_stats(tstats, wstats) and same_path(tpath, want) and tstats["moves"] >= 1
    rpath, rstats = gpu_ctx.refine_path(tpath, 7)
    f2, l2, t2, s2, r2 = gpu_ctx.pipeline_cities(blocks, 1, two_opt=1000, refine=7)
    assert (f2, l2) == (final, log) and same_path(t2, rpath) and same_stats(s2, tstats)
    assert all(r2[k] == rstats[k] for k in ("passes", "windows", "replaced", "skipped"))
    assert bits(r2["gain"]) == bits(rstats["gain"])
    # the two compose: shorter than either alone
    alone, _ = gpu_ctx.refine_path(tour, 7)
    assert tspgpu.path_length(rpath) < tspgpu.path_length(tpath) < tspgpu.path_length(alone)
    f3, l3, t3, s3 = gpu_ctx.pipeline_cities(blocks, 1, two_opt=3)
    cut, cstats = gpu_ctx.two_opt_path(tour, 2, 3)
    assert (f3, l3) == (final, log) and same_path(t3, cut) and same_stats(s3, cstats) and s3["passes"] == 3
    # both at 0 is today's call and today's tuple
    assert gpu_ctx.pipeline_cities(blocks, 1, two_opt=0, refine=0) == (final, log, tour)
    ragged = [blk[:k] for blk, k in zip(blocks, [8, 5, 7, 6] * 16)]
    fr, lr, tr = gpu_ctx.pipeline_cities_ragged(ragged, 1)
    f4, l4, t4, s4, r4 = gpu_ctx.pipeline_cities_ragged(ragged, 1, two_opt=1000, refine=7)
    tp, ts = gpu_ctx.two_opt_path(tr, 2, 1000)
    rp, rs = gpu_ctx.refine_path(tp, 7)
    assert (f4, l4) == (fr, lr) and same_path(t4, rp) and same_stats(s4, ts) and r4["replaced"] == rs["replaced"]
    assert gpu_ctx.pipeline_cities_ragged(ragged, 1, two_opt=0) == (fr, lr, tr)


def test_buffers_grow_and_are_reused_between_lengths():
    ctx = tspgpu.Context(device=0)
    try:
        for name in ("lattice-scrambled-200", "reversed-sweep-2000", "scrambled-400", "L4", "scrambled-700"):
            check_model(ctx, name)
    finally:
        ctx.close()


def test_stats_carry_the_phase_times(gpu_ctx):
    _, stats = gpu_ctx.two_opt_path(list(T.built("scrambled-700")[0]))
    assert all(stats[k] > 0.0 for k in ("grid_ms", "search_ms", "select_ms", "apply_ms"))
