"""Or-opt with a neighbour grid on the GPU (tspgpu_or_opt_path*)
against the Python model of its contract (tests/or_opt_model.py).

Nothing here has a tolerance: the path is compared id by id and coordinate
bit by coordinate bit, passes, candidates and moves exactly, `gain` as bits.
tests/test_or_opt_model.py shows that every input here (but the ones made to
move nothing) has moves applied in the model, so these are not comparisons of
untouched paths."""
import ctypes
import errno
import math
import struct

import numpy as np
import pytest

import oracle_py as O
import or_opt_model as M
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
    path, ring, seg, passes, want, wstats = M.solved(name)
    got, stats = ctx.or_opt_path(list(path), ring, seg, passes)
    assert same_stats(stats, wstats), (stats, wstats)
    assert same_path(got, want)
    return path, got, stats


@pytest.mark.parametrize("name", sorted(M.IDLE_INPUTS))
def test_nothing_to_do_matches_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert same_path(got, path) and stats["moves"] == 0


@pytest.mark.parametrize("name", sorted(M.MOVING_INPUTS))
def test_inputs_match_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert stats["moves"] >= 1 and tspgpu.path_length(got) < tspgpu.path_length(path)
    assert sorted(got) == sorted(path) and got[0] == path[0] and got[-1] == path[-1]


@pytest.mark.parametrize("name", sorted(M.CUT_INPUTS))
def test_runs_cut_by_max_passes_match_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert stats["passes"] == M.built(name)[3] and stats["moves"] >= 1


@pytest.mark.parametrize("name", sorted(M.SCALED_INPUTS))
def test_scaled_inputs_match_the_model(gpu_ctx, name):
    """The same order as the base input and its gain times the scale exactly
    (tests/test_or_opt_model.py): a mismatch here is the distance code's."""
    check_model(gpu_ctx, name)


def on_device(ctx, path, ring, seg, passes):
    """The device form on an upload of `path` -> (rc or stats, the path after)."""
    arr, L, _ = tspgpu.cities_array([path])
    d_path = ctx.upload(np.frombuffer(arr, np.uint8))
    try:
        try:
            out = ctx.or_opt_path_device(d_path, L, ring, seg, passes, ctx.stream)
        except tspgpu.TspGpuError as err:
            out = err.code
        raw = ctx.download(d_path, (L,), tspgpu.CITY_DTYPE)
    finally:
        ctx.free(d_path)
    return out, [(int(c["id"]), float(c["x"]), float(c["y"])) for c in raw]


@pytest.mark.parametrize("name", ["2opt:scrambled-400", "stray-backward-2000", "L3", "L6"])
def test_host_form_equals_device_form(gpu_ctx, name):
    path, ring, seg, passes, want, wstats = M.solved(name)
    stats, got = on_device(gpu_ctx, path, ring, seg, passes)
    assert same_stats(stats, wstats) and same_path(got, want)


def test_refused_paths_return_the_codes_and_stay(gpu_ctx):
    base = list(M.built("scrambled-400")[0])
    cases = []
    for bad in (math.nan, math.inf, -math.inf):
        for at, axis in ((0, 1), (137, 2), (399, 1)):
            path = [list(c) for c in base]
            path[at][axis] = bad
            cases.append(([tuple(c) for c in path], -errno.EINVAL))
    cases.append((T.scaled(base, 502), -errno.ERANGE))  # finite coordinates, the squared extents' sum is not
    cases.append(([(0, math.nan, 1.0), (1, 2.0, 3.0)], -errno.EINVAL))  # validated also where nothing could move
    for path, code in cases:
        assert M.or_opt(path)[1] == code
        rc, after = on_device(gpu_ctx, path, 2, 3, 1000)
        assert rc == code
        assert all(a[0] == b[0] and bits(a[1]) == bits(b[1]) and bits(a[2]) == bits(b[2]) for a, b in zip(after, path))
        # the host form writes neither the output nor the stats
        arr, L, _ = tspgpu.cities_array([path])
        out = (tspgpu.City * L)()
        st = tspgpu.OrOptStats(passes=7)
        assert tspgpu.lib().tspgpu_or_opt_path(gpu_ctx.handle, arr, L, 2, 3, 1000, out, ctypes.byref(st)) == code
        assert st.passes == 7 and all(c.id == 0 and c.x == 0.0 for c in out)
    # the context still works
    check_model(gpu_ctx, "scrambled-400-cut3")


def test_bad_arguments_on_a_live_context(gpu_ctx):
    path = list(M.built("L6")[0])
    for ring, seg, passes in ((0, 3, 8), (5, 3, 8), (2, 3, 0), (-1, 3, 8), (2, 0, 8), (2, 4, 8), (2, -1, 8)):
        with pytest.raises(tspgpu.TspGpuError) as err:
            gpu_ctx.or_opt_path(path, ring, seg, passes)
        assert err.value.code == -errno.EINVAL


def test_in_place_host_form(gpu_ctx):
    path, ring, seg, passes, want, wstats = M.solved("2opt:closed-tour-251")
    arr, L, _ = tspgpu.cities_array([path])
    st = tspgpu.OrOptStats()
    assert tspgpu.lib().tspgpu_or_opt_path(gpu_ctx.handle, arr, L, ring, seg, passes, arr, ctypes.byref(st)) == 0
    assert same_stats(st.as_dict(), wstats) and same_path([(arr[i].id, arr[i].x, arr[i].y) for i in range(L)], want)
    assert tspgpu.lib().tspgpu_or_opt_path(gpu_ctx.handle, arr, L, ring, seg, passes, arr, None) == 0  # stats may be NULL


def test_pipeline_keywords_are_the_separate_calls(gpu_ctx):
    blocks = O.generate(8, 64, 1000, 1000)
    final, log, tour = gpu_ctx.pipeline_cities(blocks, 1)
    tpath, tstats = gpu_ctx.two_opt_path(tour, 2, 1000)
    opath, ostats = gpu_ctx.or_opt_path(tpath, 2, 3, 1000)
    # (the model's shared run of this case starts from the 2-opt model's result on the oracle's merge)
    shared, ring, seg, passes, want, wstats = M.solved("2opt:generator-8x64")
    if not same_path(tpath, shared):
        want, wstats = M.or_opt(tpath, ring, seg, passes)
    assert same_stats(ostats, wstats) and same_path(opath, want) and ostats["moves"] >= 1
    rpath, rstats = gpu_ctx.refine_path(opath, 7)
    f2, l2, t2, s2, o2, r2 = gpu_ctx.pipeline_cities(blocks, 1, two_opt=1000, or_opt=1000, refine=7)
    assert (f2, l2) == (final, log) and same_path(t2, rpath) and same_stats(s2, tstats) and same_stats(o2, ostats)
    assert all(r2[k] == rstats[k] for k in ("passes", "windows", "replaced", "skipped"))
    assert bits(r2["gain"]) == bits(rstats["gain"])
    assert tspgpu.path_length(rpath) <= tspgpu.path_length(opath) < tspgpu.path_length(tpath)
    # alone, and cut
    f3, l3, t3, o3 = gpu_ctx.pipeline_cities(blocks, 1, or_opt=3)
    cut, cstats = gpu_ctx.or_opt_path(tour, 2, 3, 3)
    assert (f3, l3) == (final, log) and same_path(t3, cut) and same_stats(o3, cstats) and o3["passes"] == 3
    # at 0 it is today's call and today's tuple
    assert gpu_ctx.pipeline_cities(blocks, 1, two_opt=0, or_opt=0, refine=0) == (final, log, tour)
    ragged = [blk[:k] for blk, k in zip(blocks, [8, 5, 7, 6] * 16)]
    fr, lr, tr = gpu_ctx.pipeline_cities_ragged(ragged, 1)
    f4, l4, t4, s4, o4, r4 = gpu_ctx.pipeline_cities_ragged(ragged, 1, two_opt=1000, or_opt=1000, refine=7)
    tp, ts = gpu_ctx.two_opt_path(tr, 2, 1000)
    op, os_ = gpu_ctx.or_opt_path(tp, 2, 3, 1000)
    rp, rs = gpu_ctx.refine_path(op, 7)
    assert (f4, l4) == (fr, lr) and same_path(t4, rp) and same_stats(s4, ts) and same_stats(o4, os_)
    assert r4["replaced"] == rs["replaced"]
    assert gpu_ctx.pipeline_cities_ragged(ragged, 1, or_opt=0) == (fr, lr, tr)


def test_one_context_alternates_or_opt_and_two_opt_between_lengths():
    """The two stages share the state and grid buffers: growing and shrinking
    lengths in turn, and both still match their models."""
    ctx = tspgpu.Context(device=0)
    try:
        for oname, tname in (("lattice-scrambled-200", "scrambled-700"), ("stray-forward-2000", "L4"),
                             ("2opt:scrambled-400", "reversed-sweep-2000"), ("L5", "lattice-scrambled-200"),
                             ("2opt:scrambled-700", "bow-tie")):
            check_model(ctx, oname)
            path, ring, passes, want, wstats = T.solved(tname)
            got, stats = ctx.two_opt_path(list(path), ring, passes)
            assert same_stats(stats, wstats) and same_path(got, want)
    finally:
        ctx.close()


def test_stats_carry_the_phase_times(gpu_ctx):
    _, stats = gpu_ctx.or_opt_path(list(M.built("2opt:scrambled-700")[0]))
    assert all(stats[k] > 0.0 for k in ("grid_ms", "search_ms", "select_ms", "apply_ms"))
