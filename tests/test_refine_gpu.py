"""Window refinement of a tour on the GPU (tspgpu_refine_path*)
against the Python model of its contract (tests/refine_model.py, on the CPU
oracle alone).

Nothing here has a tolerance: the refined path is compared id by id and
coordinate bit by coordinate bit, the stats entry by entry, `gain` as bits.
tests/test_refine_model.py shows that every input here (but the ones made to
replace nothing) has windows replaced in the model, so these are not
comparisons of untouched paths."""
import struct

import numpy as np
import pytest

import oracle_py as O
import refine_model as R
import tspgpu

pytestmark = pytest.mark.gpu

KEYS = ("passes", "windows", "replaced", "skipped", "gain")


def bits(v):
    return struct.pack("<d", v)


def same_path(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and bits(x[1]) == bits(y[1]) and bits(x[2]) == bits(y[2])
                                    for x, y in zip(a, b))


def same_stats(got, want):
    return all(got[k] == want[k] for k in KEYS[:4]) and bits(got["gain"]) == bits(want["gain"])


def check_model(ctx, path, m, passes, want_path, want_stats):
    got, stats = ctx.refine_path(list(path), m, passes)
    assert same_stats(stats, want_stats), (stats, want_stats)
    assert same_path(got, want_path)
    return got, stats


@pytest.mark.parametrize("name", sorted(R.SMALL_INPUTS))
def test_small_lengths_match_the_model(gpu_ctx, name):
    path, m, passes, want, wstats = R.refined(name)
    check_model(gpu_ctx, path, m, passes, want, wstats)


@pytest.mark.parametrize("name", ["scrambled-400-m7", "scrambled-600-m15", "line-300-m7", "lattice-scrambled-200-m7"])
def test_inputs_match_the_model(gpu_ctx, name):
    path, m, passes, want, wstats = R.refined(name)
    got, stats = check_model(gpu_ctx, path, m, passes, want, wstats)
    assert stats["replaced"] >= 1 and tspgpu.path_length(got) < tspgpu.path_length(path)
    assert sorted(got) == sorted(path) and got[0] == path[0] and got[-1] == path[-1]


def test_tie_only_lattice_is_left_alone(gpu_ctx):
    path, m, passes, want, wstats = R.refined(R.TIE_INPUT[0])
    got, stats = check_model(gpu_ctx, path, m, passes, want, wstats)
    assert stats["replaced"] == 0 and stats["windows"] > 0 and same_path(got, path)


def test_outlier_windows_are_skipped(gpu_ctx):
    path, m, passes, want, wstats = R.refined("outlier-200-m7")
    got, stats = check_model(gpu_ctx, path, m, passes, want, wstats)
    assert stats["skipped"] >= 1 and stats["replaced"] >= 1


def test_m12_from_one_window_per_cu_runs_variant_6(gpu_ctx):
    cus, _ = gpu_ctx.device_info()
    path, m, passes = R.wide_input(cus)
    want, wstats = R.refine(path, m, passes)
    check_model(gpu_ctx, path, m, passes, want, wstats)
    assert gpu_ctx.last_variant() == 6 and wstats["replaced"] >= 1


def test_pipeline_tour_refined(gpu_ctx):
    blocks = O.generate(8, 64, 1000, 1000)
    final, log, tour = gpu_ctx.pipeline_cities(blocks, 1)
    # (the model's shared run of this case starts from the oracle's merge of the same batch)
    shared, m, passes, want, wstats = R.refined("generator-8x64-m15")
    if not same_path(tour, shared):
        want, wstats = R.refine(tour, m, passes)
    assert wstats["replaced"] >= 1
    got, stats = check_model(gpu_ctx, tour, m, passes, want, wstats)
    assert tspgpu.path_length(got) < tspgpu.path_length(tour)
    assert sorted(c[0] for c in got) == sorted(c[0] for c in tour)
    assert got[0] == tour[0] and got[-1] == tour[-1]
    # the keyword is the two-step call; at its default the call is today's
    f2, l2, t2, s2 = gpu_ctx.pipeline_cities(blocks, 1, refine=15)
    assert (f2, l2) == (final, log) and same_path(t2, got) and same_stats(s2, stats)
    assert gpu_ctx.pipeline_cities(blocks, 1, refine=0) == (final, log, tour)
    ragged = [blk[:k] for blk, k in zip(blocks, [8, 5, 7, 6] * 16)]
    fr, lr, tr = gpu_ctx.pipeline_cities_ragged(ragged, 1)
    f3, l3, t3, s3 = gpu_ctx.pipeline_cities_ragged(ragged, 1, refine=7)
    rp, rs = gpu_ctx.refine_path(tr, 7)
    assert (f3, l3) == (fr, lr) and same_path(t3, rp) and same_stats(s3, rs)


def test_host_form_equals_device_form(gpu_ctx):
    path, m, passes, want, wstats = R.refined("scrambled-400-m7")
    arr, L, _ = tspgpu.cities_array([path])
    d_path = gpu_ctx.upload(np.frombuffer(arr, np.uint8))
    try:
        stats = gpu_ctx.refine_path_device(d_path, L, m, passes, gpu_ctx.stream)
        raw = gpu_ctx.download(d_path, (L,), tspgpu.CITY_DTYPE)
    finally:
        gpu_ctx.free(d_path)
    got = [(int(c["id"]), float(c["x"]), float(c["y"])) for c in raw]
    assert same_stats(stats, wstats) and same_path(got, want)


def test_path_length_equals_the_python_fold(gpu_ctx):
    for name in ("scrambled-400-m7", "line-300-m7", "lattice-scrambled-200-m7"):
        path = R.refined(name)[0]
        assert bits(tspgpu.path_length(path)) == bits(R.path_length(path))
    assert tspgpu.path_length([(1, 2.0, 3.0)]) == 0.0
