"""K1 -> K3 on the device and the merged tour, the part that needs no GPU: the
entry points are exported with the documented signatures, the argument errors
that are decided before any device work are refused and nothing is written,
and the binding carries the methods.  (tests/test_abi.py checks the header
side: every declared symbol is exported.)"""
import ctypes
import errno
import inspect
import os
import re

import numpy as np

import tspgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tspgpu_reduce_path", "tspgpu_reduce_device", "tspgpu_pipeline_cities", "tspgpu_reduce_device_last_ms"}
EINVAL = -errno.EINVAL

# parameter types, in order, as include/tspgpu.h declares them
SIGNATURES = {
    "tspgpu_reduce_path": ["tspgpu_ctx *", "const tspgpu_city *", "int", "const double *", "int", "int", "double *",
                           "tspgpu_city *", "int", "int *", "char *", "int"],
    "tspgpu_reduce_device": ["tspgpu_ctx *", "const tspgpu_city *", "const int32_t *", "const double *",
                             "const int32_t *", "int", "int", "int", "double *", "tspgpu_city *", "int", "int *",
                             "char *", "int", "void *"],
    "tspgpu_pipeline_cities": ["tspgpu_ctx *", "const tspgpu_city *", "int", "int", "int", "double *",
                               "tspgpu_city *", "int", "int *", "char *", "int"],
}


def test_symbols_exported_with_the_documented_signatures():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NAMES)
    assert NAMES <= set(tspgpu.EXPORTED_SYMBOLS)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tspgpu.h")).read(), flags=re.S)
    for name, want in SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        got = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(1).split(",")]
        assert got == want, (name, got)
        # the binding passes as many arguments as the header declares
        assert len(getattr(tspgpu.lib(), name).argtypes) == len(want), name


def _host_args(B=2, L=4):
    paths = (tspgpu.City * (B * L))()
    for k in range(B * L):
        paths[k].id, paths[k].x, paths[k].y = k, float(k), 2.0 * k
    costs = np.full(B, 7.0)
    return paths, costs


def test_reduce_path_argument_errors_need_no_device():
    L = tspgpu.lib()
    paths, costs = _host_args()
    out = (tspgpu.City * 16)()
    final, plen = ctypes.c_double(7.0), ctypes.c_int(7)
    log = ctypes.create_string_buffer(b"x", 64)

    def call(ctx=None, p=paths, LL=4, c=costs, B=2, P=1, f=final, o=out, cap=16, pl=plen):
        return L.tspgpu_reduce_path(ctx, p, LL, tspgpu._dp(c) if c is not None else None, B, P,
                                    ctypes.byref(f) if f is not None else None, o, cap,
                                    ctypes.byref(pl) if pl is not None else None, log, len(log))

    assert call() == EINVAL  # NULL context
    fake = ctypes.c_void_p(1)  # (never dereferenced: the checks below come first)
    assert call(fake, p=None) == EINVAL
    assert call(fake, c=None) == EINVAL
    assert call(fake, f=None) == EINVAL
    assert call(fake, pl=None) == EINVAL
    assert call(fake, B=0) == EINVAL
    assert call(fake, B=2, P=3) == EINVAL  # nblocks < nprocs
    assert call(fake, P=0) == EINVAL
    assert call(fake, LL=1) == EINVAL
    assert call(fake, cap=-1) == EINVAL
    assert call(fake, o=None, cap=4) == EINVAL
    assert final.value == 7.0 and plen.value == 7 and all(c.id == 0 for c in out)


def test_device_and_pipeline_argument_errors_need_no_device():
    L = tspgpu.lib()
    cities, n, B = tspgpu.cities_array([[(i, float(i), 2.0 * i) for i in range(5)]] * 2)
    addr = ctypes.addressof(cities)
    out = (tspgpu.City * 16)()
    final, plen = ctypes.c_double(7.0), ctypes.c_int(7)
    fin, pl = ctypes.byref(final), ctypes.byref(plen)
    fake = ctypes.c_void_p(1)
    log = ctypes.create_string_buffer(64)
    # (ctx, n, nblocks, nprocs)
    bad = [(None, 5, 2, 1), (fake, 1, 2, 1), (fake, 21, 2, 1), (fake, 0, 2, 1), (fake, 5, 0, 1), (fake, 5, -1, 1),
           (fake, 5, 2, 3), (fake, 5, 2, 0)]
    for ctx, nn, nb, P in bad:
        assert L.tspgpu_reduce_device(ctx, addr, addr, addr, addr, nn, nb, P, fin, None, 0, pl, log, 64,
                                      None) == EINVAL, (nn, nb, P)
        assert L.tspgpu_pipeline_cities(ctx, cities, nn, nb, P, fin, out, 16, pl, log, 64) == EINVAL, (nn, nb, P)
    # NULL pointers, a negative capacity, a capacity without a destination
    assert L.tspgpu_reduce_device(fake, None, addr, addr, addr, 5, 2, 1, fin, None, 0, pl, log, 64, None) == EINVAL
    assert L.tspgpu_reduce_device(fake, addr, None, addr, addr, 5, 2, 1, fin, None, 0, pl, log, 64, None) == EINVAL
    assert L.tspgpu_reduce_device(fake, addr, addr, None, addr, 5, 2, 1, fin, None, 0, pl, log, 64, None) == EINVAL
    assert L.tspgpu_reduce_device(fake, addr, addr, addr, addr, 5, 2, 1, None, None, 0, pl, log, 64, None) == EINVAL
    assert L.tspgpu_reduce_device(fake, addr, addr, addr, addr, 5, 2, 1, fin, None, 0, None, log, 64, None) == EINVAL
    assert L.tspgpu_reduce_device(fake, addr, addr, addr, addr, 5, 2, 1, fin, None, 4, pl, log, 64, None) == EINVAL
    assert L.tspgpu_reduce_device(fake, addr, addr, addr, addr, 5, 2, 1, fin, addr, -1, pl, log, 64, None) == EINVAL
    assert L.tspgpu_pipeline_cities(fake, None, 5, 2, 1, fin, out, 16, pl, log, 64) == EINVAL
    assert L.tspgpu_pipeline_cities(fake, cities, 5, 2, 1, None, out, 16, pl, log, 64) == EINVAL
    assert L.tspgpu_pipeline_cities(fake, cities, 5, 2, 1, fin, out, 16, None, log, 64) == EINVAL
    assert L.tspgpu_pipeline_cities(fake, cities, 5, 2, 1, fin, None, 16, pl, log, 64) == EINVAL
    assert L.tspgpu_pipeline_cities(fake, cities, 5, 2, 1, fin, out, -1, pl, log, 64) == EINVAL
    assert L.tspgpu_reduce_device_last_ms(None, None) == EINVAL
    assert final.value == 7.0 and plen.value == 7 and all(c.id == 0 for c in out)


def test_binding_has_the_methods():
    for name in ("reduce_path", "reduce_device", "pipeline_cities", "reduce_device_last_ms", "reduce"):
        assert callable(getattr(tspgpu.Context, name, None)), name
    p = inspect.signature(tspgpu.Context.reduce_device).parameters
    assert list(p)[1:8] == ["d_cities_ptr", "d_tour_ptr", "d_cost_ptr", "d_status_ptr", "n", "B", "nprocs"]
    assert (p["d_path_ptr"].default, p["path_cap"].default, p["stream_ptr"].default) == (0, 0, 0)
    assert list(inspect.signature(tspgpu.Context.reduce_path).parameters)[1:4] == ["paths", "costs", "nprocs"]
    assert list(inspect.signature(tspgpu.Context.pipeline_cities).parameters)[1:3] == ["blocks", "nprocs"]
    # Context.reduce is what it was
    assert list(inspect.signature(tspgpu.Context.reduce).parameters) == ["self", "paths", "costs", "nprocs"]


def test_two_city_cases_terminate_in_the_reference():
    """The premise of the n = 2 cases of tests/test_pipeline_gpu.py, on the CPU:
    the oracle's tour of a 2-city block is [1, 0] and the host replay of the
    reference's merge returns 0 for those (B, P)."""
    import oracle_py as O
    import test_pipeline_gpu as G

    for B, P in G.TWO_CITY:
        blocks = G.two_city_blocks(B)
        assert all(O.solve_block(O.distance_matrix(blk))[1] == [1, 0] for blk in blocks)
        sols = [([blk[1], blk[0]], O.solve_block(O.distance_matrix(blk))[0]) for blk in blocks]
        assert G.host_reduce_rc(sols, P)[0] == 0, (B, P)
