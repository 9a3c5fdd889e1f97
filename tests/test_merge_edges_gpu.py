"""K3 (csrc/merge.hip, csrc/paths.hip) off the generator's coordinates:
negative, translated and rescaled planes, a bounding box far wider than the
swap-cost spread, and more tied pairs than the candidate buffer holds, against
the host parity layer (tsphost_merge, tsphost_reduce) as in
tests/test_merge_gpu.py.  Costs are compared as floats with ==, paths by id.

Every input stays inside K3's domain (include/tspgpu.h): finite coordinates,
coordinate-difference squares zero or in [2^-900, 2^1000], a minimum swap
cost below INT_MAX.  tests/test_coord_families.py asserts that, and the tied-
pair counts of the two overflow cases, on the CPU."""
import ctypes
import functools

import numpy as np
import pytest

import coord_families as F
import tspgpu
from test_host import H, _solve_all, city_array
from test_merge_gpu import _host_reduce, host_merge
from test_pipeline_gpu import bits, host_form

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("outlier",) + F.K3_FAMILIES)
def test_growing_folds_match_host(gpu_ctx, name):
    """test_merge_matches_host's loop (40 merges, blocks of 2..16 cities) with
    the paths through a family; "outlier": clustered cities and one 10^8 away:
    in 33 of the 40 merges the candidate window (eps2 ~ 0.01) holds pairs
    whose exact swap costs differ, and the host has to pick among them."""
    acc, acc_c, blocks = F.growing_fold(name)
    hacc, hacc_c = acc, acc_c
    for step, (p2, c2) in enumerate(blocks):
        hres, hcost = host_merge(hacc, hacc_c, p2, c2)
        if hres is None:
            with pytest.raises(tspgpu.TspGpuError) as e:
                gpu_ctx.merge(acc, acc_c, p2, c2)
            assert e.value.code == -35  # -EDEADLK: the reference loops forever here
            continue
        acc, acc_c = gpu_ctx.merge(acc, acc_c, p2, c2)
        hacc, hacc_c = hres, hcost
        assert acc_c == hacc_c and [c[0] for c in acc] == [c[0] for c in hacc], step
        assert bits(acc) == bits(hacc), step


@pytest.mark.parametrize("points", (2, 1))
def test_merge_with_more_tied_pairs_than_the_candidate_buffer(gpu_ctx, points):
    """67613 (two points) and 88417 (one) pairs tie at the minimum: the general
    path's candidate list overflows and the host rescans every pair."""
    p1, c1, p2, c2 = F.overflow_merge(points)
    h, hc = host_merge(p1, c1, p2, c2)
    g, gc = gpu_ctx.merge(p1, c1, p2, c2)
    assert gc == hc and [c[0] for c in g] == [c[0] for c in h]


@functools.lru_cache(maxsize=None)
def _overflow_fold_reference():
    """The blocks' oracle solutions, _host_reduce's answer at P = 1 and, for the
    final path (the cost of coincident cities is 0 and one rank logs nothing),
    the ids of the same fold through tsphost_merge; computed once."""
    sols = _solve_all(F.overflow_fold_blocks())
    hf, hlog = _host_reduce(sols, 1)
    acc, cost = np.array(sols[0][0], dtype=tspgpu.CITY_DTYPE), sols[0][1]
    for p2, c2 in sols[1:]:
        a1 = (tspgpu.City * len(acc)).from_buffer_copy(acc.tobytes())
        out = (tspgpu.City * (len(acc) + len(p2)))()
        c = ctypes.c_double()
        L = H.tsphost_merge(a1, len(acc), cost, city_array(p2), len(p2), c2, out, ctypes.byref(c))
        assert L == len(acc) + len(p2) - 1
        acc, cost = np.frombuffer(out, dtype=tspgpu.CITY_DTYPE, count=L).copy(), c.value
    assert cost == hf
    return sols, hf, hlog, acc["id"].tolist()


@pytest.mark.parametrize("persist", (1, 0))
def test_fold_with_more_tied_pairs_than_the_candidate_buffer(gpu_ctx, knobs, persist):
    """914 coincident 8-city blocks at P = 1: the last three merges have more
    than 65536 tied pairs (fold_pick_kernel's nc > kCandCap), by the
    persistent fold handing over at 4096 cities (default) and by the per-merge
    kernels alone (K3_PERSIST = 0).  Every one of the 913 merges is a tie the
    host resolves, one round trip each, so a case takes several seconds."""
    sols, hf, hlog, hids = _overflow_fold_reference()
    paths, costs = [p for p, _ in sols], [c for _, c in sols]
    if not persist:
        knobs.set("K3_PERSIST", "0")
    final, log, path = gpu_ctx.reduce_path(paths, costs, 1)
    assert final == hf, (final, hf)
    assert sorted(log.splitlines()) == sorted(hlog.splitlines())
    assert [c[0] for c in path] == hids


@pytest.mark.parametrize("name", ("neg", "shift40"))
@pytest.mark.parametrize("kind,n,B,P", [("lattice", 6, 48, 1), ("random", 8, 300, 8)])
def test_persistent_fold_matches_host_under_families(gpu_ctx, knobs, kind, n, B, P, name):
    sols = _solve_all(F.family_fold_blocks(kind, n, B, P, name))
    hf, hlog = _host_reduce(sols, P)
    paths, costs = [p for p, _ in sols], [c for _, c in sols]
    f1, log1 = gpu_ctx.reduce(paths, costs, P)
    knobs.set("K3_PERSIST", "0")
    f0, log0 = gpu_ctx.reduce(paths, costs, P)
    assert f1 == hf and f0 == hf, (f1, f0, hf)
    assert log1 == log0 and sorted(log1.splitlines()) == sorted(hlog.splitlines())


@pytest.mark.parametrize("P", (1, 3))
@pytest.mark.parametrize("name", ("neg", "scale20"))
def test_device_extrema_give_the_host_handoffs_answer(gpu_ctx, name, P):
    """pipeline_cities is the one route on which Dmax comes from the device's
    order keys of the coordinates (negative ones and -0.0 under neg): cost,
    log and the final path's bits equal solve_cities + reduce_path."""
    blocks = F.block_lists(F.cities(name, 8, 64, pick=False))
    hcost, hlog, hpath = host_form(gpu_ctx, blocks, P)
    cost, log, path = gpu_ctx.pipeline_cities(blocks, P)
    assert np.float64(cost).hex() == np.float64(hcost).hex() and log == hlog
    assert bits(path) == bits(hpath)
