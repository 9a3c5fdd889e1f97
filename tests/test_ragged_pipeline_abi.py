"""Ragged blocks end to end, the part that needs no GPU: the six
entry points are exported with the header's parameter lists, every call-level
error is refused with a fake non-NULL context before anything is dereferenced
or written, and the binding carries the methods."""
import ctypes
import errno
import inspect
import os
import re

import numpy as np

import tspgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -errno.EINVAL

# parameter types, in order, as include/tspgpu.h declares them
SIGNATURES = {
    "tspgpu_distance_matrix_ragged_device": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "int",
                                             "double *", "void *"],
    "tspgpu_solve_cities_ragged_device": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "int", "double *",
                                          "int32_t *", "int", "int32_t *", "void *"],
    "tspgpu_solve_cities_ragged": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "int", "double *",
                                   "int32_t *", "int", "int32_t *"],
    "tspgpu_reduce_ragged_device": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "const int32_t *", "int",
                                    "const double *", "const int32_t *", "int", "int", "double *", "tspgpu_city *",
                                    "int", "int *", "char *", "int", "void *"],
    "tspgpu_reduce_ragged": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "const double *", "int", "int",
                             "double *", "tspgpu_city *", "int", "int *", "char *", "int"],
    "tspgpu_pipeline_cities_ragged": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "int", "int",
                                      "double *", "tspgpu_city *", "int", "int *", "char *", "int"],
}
BAD_N = [[5, 0, 5], [5, 21, 5], [5, -3, 5], [5, 1, 5]]  # (1 is in range for the distance form only)


def test_symbols_exported_with_the_documented_signatures():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in SIGNATURES)
    assert set(SIGNATURES) <= set(tspgpu.EXPORTED_SYMBOLS)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tspgpu.h")).read(), flags=re.S)
    for name, want in SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        got = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(1).split(",")]
        assert got == want, (name, got)
        # the binding passes as many arguments as the header declares
        assert len(getattr(tspgpu.lib(), name).argtypes) == len(want), name


def _ns(n):
    return np.ascontiguousarray(n, dtype=np.int32)


class Outputs:
    """Host outputs pre-filled with 7: a refused call writes none of them."""

    def __init__(self):
        self.cost = np.full(8, 7.0)
        self.tour = np.full(8 * 32, 7, dtype=np.int32)
        self.status = np.full(8, 7, dtype=np.int32)
        self.out = (tspgpu.City * 64)()
        self.final, self.plen = ctypes.c_double(7.0), ctypes.c_int(7)
        self.log = ctypes.create_string_buffer(64)

    def untouched(self):
        return ((self.cost == 7.0).all() and (self.tour == 7).all() and (self.status == 7).all()
                and all(c.id == 0 for c in self.out) and self.final.value == 7.0 and self.plen.value == 7)


def test_solve_and_distance_forms_refuse_bad_arguments():
    L = tspgpu.lib()
    cities = (tspgpu.City * 64)()
    addr = ctypes.addressof(cities)
    o = Outputs()
    fake = ctypes.c_void_p(1)  # (never dereferenced: the checks come first)
    good = _ns([5, 7, 5])

    def dist(ctx=fake, c=addr, n=good, B=3, d=addr):
        return L.tspgpu_distance_matrix_ragged_device(ctx, c, tspgpu._ip(n) if n is not None else None, B, d, None)

    def dev(ctx=fake, c=addr, n=good, B=3, cost=addr, tour=addr, stride=8, st=addr):
        return L.tspgpu_solve_cities_ragged_device(ctx, c, tspgpu._ip(n) if n is not None else None, B, cost, tour,
                                                   stride, st, None)

    def host(ctx=fake, c=cities, n=good, B=3, cost=o.cost, tour=o.tour, stride=8, st=o.status):
        return L.tspgpu_solve_cities_ragged(ctx, c, tspgpu._ip(n) if n is not None else None, B,
                                            tspgpu._dp(cost) if cost is not None else None,
                                            tspgpu._ip(tour) if tour is not None else None, stride,
                                            tspgpu._ip(st) if st is not None else None)

    for f in (dist, dev, host):
        assert f(ctx=None) == EINVAL
        assert f(B=-1) == EINVAL
        assert f(c=None) == EINVAL
        assert f(n=None) == EINVAL
        assert f(B=0) == 0  # nothing to do
        assert f(ctx=None, B=0) == EINVAL
    assert dist(d=None) == EINVAL
    for f in (dev, host):
        assert f(cost=None) == EINVAL
        assert f(tour=None) == EINVAL
        assert f(st=None) == EINVAL
        assert f(stride=7) == EINVAL  # max n + 1 = 8
        assert f(n=_ns([5, 20, 5]), stride=20) == EINVAL
    # any n[b] out of range: the packed layout is undefined
    for bad in BAD_N:
        n = _ns(bad)
        assert dev(n=n) == EINVAL and host(n=n) == EINVAL, bad
        if bad[1] != 1:
            assert dist(n=n) == EINVAL, bad
    assert o.untouched()


def test_reduce_and_pipeline_forms_refuse_bad_arguments():
    L = tspgpu.lib()
    cities = (tspgpu.City * 64)()
    for k in range(64):
        cities[k].id, cities[k].x, cities[k].y = k, float(k), 2.0 * k
    addr = ctypes.addressof(cities)
    o = Outputs()
    fin, pl = ctypes.byref(o.final), ctypes.byref(o.plen)
    fake = ctypes.c_void_p(1)
    good = _ns([5, 7, 5])
    costs = np.full(3, 7.0)

    def dev(ctx=fake, c=addr, n=good, tour=addr, stride=8, cost=addr, B=3, P=1, f=fin, out=None, cap=0, p=pl):
        return L.tspgpu_reduce_ragged_device(ctx, c, tspgpu._ip(n) if n is not None else None, tour, stride, cost,
                                             addr, B, P, f, out, cap, p, o.log, 64, None)

    def host(ctx=fake, c=cities, n=good, cost=costs, B=3, P=1, f=fin, out=o.out, cap=64, p=pl):
        return L.tspgpu_reduce_ragged(ctx, c, tspgpu._ip(n) if n is not None else None,
                                      tspgpu._dp(cost) if cost is not None else None, B, P, f, out, cap, p, o.log, 64)

    def pipe(ctx=fake, c=cities, n=good, B=3, P=1, f=fin, out=o.out, cap=64, p=pl):
        return L.tspgpu_pipeline_cities_ragged(ctx, c, tspgpu._ip(n) if n is not None else None, B, P, f, out, cap, p,
                                               o.log, 64)

    for f in (dev, host, pipe):
        assert f(ctx=None) == EINVAL
        assert f(c=None) == EINVAL
        assert f(n=None) == EINVAL
        assert f(B=0) == EINVAL and f(B=-1) == EINVAL  # nblocks < 1
        assert f(P=0) == EINVAL
        assert f(P=4) == EINVAL  # nblocks < nprocs
        assert f(f=None) == EINVAL
        assert f(p=None) == EINVAL
        assert f(cap=-1) == EINVAL
        assert f(out=None, cap=4) == EINVAL  # a capacity with no destination
    assert dev(tour=None) == EINVAL and dev(cost=None) == EINVAL
    assert dev(stride=7) == EINVAL
    assert host(cost=None) == EINVAL
    for bad in BAD_N:
        n = _ns(bad)
        assert dev(n=n) == EINVAL and pipe(n=n) == EINVAL, bad
        if bad[1] < 2:  # (the host front takes path lengths: any len[b] >= 2 is in range)
            assert host(n=n) == EINVAL, bad
    assert o.untouched()


def test_binding_has_the_methods():
    for name in ("distance_matrix_ragged_device", "solve_cities_ragged", "solve_cities_ragged_device",
                 "reduce_ragged", "reduce_ragged_device", "pipeline_cities_ragged"):
        assert callable(getattr(tspgpu.Context, name, None)), name
    assert callable(tspgpu.cities_array_ragged)
    arr, n = tspgpu.cities_array_ragged([[(1, 0.5, 1.5)] * 3, [(9, 2.0, 3.0)] * 2])
    assert n.tolist() == [3, 2] and n.dtype == np.int32
    assert [(arr[k].id, arr[k].x, arr[k].y) for k in range(5)] == [(1, 0.5, 1.5)] * 3 + [(9, 2.0, 3.0)] * 2
    p = inspect.signature(tspgpu.Context.reduce_ragged_device).parameters
    assert list(p)[1:8] == ["d_cities_ptr", "n", "d_tour_ptr", "tour_stride", "d_cost_ptr", "d_status_ptr", "nprocs"]
    assert (p["d_path_ptr"].default, p["path_cap"].default, p["stream_ptr"].default) == (0, 0, 0)
    assert list(inspect.signature(tspgpu.Context.reduce_ragged).parameters)[1:4] == ["paths", "costs", "nprocs"]
    assert list(inspect.signature(tspgpu.Context.pipeline_cities_ragged).parameters)[1:3] == ["blocks", "nprocs"]
