"""Fixed-end paths and the window refinement, the part that needs no GPU: the
entry points are exported, the argument errors that are decided before any
device work are refused and nothing is written, tspgpu_path_length (host code)
folds as the Python model does, and the binding carries the methods.
(tests/test_abi.py checks the header side: every declared symbol is exported.)"""
import ctypes
import errno
import inspect
import struct

import numpy as np

import refine_model as R
import tspgpu

NAMES = {"tspgpu_solve_paths", "tspgpu_solve_paths_device", "tspgpu_solve_paths_cities",
         "tspgpu_solve_paths_cities_device", "tspgpu_refine_path", "tspgpu_refine_path_device", "tspgpu_path_length"}
EINVAL = -errno.EINVAL


def test_symbols_exported():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NAMES)
    assert NAMES <= set(tspgpu.EXPORTED_SYMBOLS)


def test_null_context_refused_without_a_device():
    L = tspgpu.lib()
    cities, w, B = tspgpu.cities_array([[(i, float(i), 2.0 * i) for i in range(6)]] * 2)
    dist = np.full((2, 6, 6), 7.0)
    cost = np.full(2, 7.0)
    order = np.full((2, 6), 7, dtype=np.int32)
    status = np.full(2, 7, dtype=np.int32)
    out = (tspgpu.City * 12)()
    st = tspgpu.RefineStats(passes=7)
    addr = ctypes.addressof(cities)
    for ww, nb in ((6, 2), (3, 2), (21, 2), (6, -1), (6, 0)):
        # (the context is checked first, also with nothing to do)
        for dtype in (tspgpu.F64, tspgpu.I32, 5):
            assert L.tspgpu_solve_paths(None, dist.ctypes.data, dtype, ww, nb, cost.ctypes.data, tspgpu._ip(order),
                                        tspgpu._ip(status)) == EINVAL
            assert L.tspgpu_solve_paths_device(None, dist.ctypes.data, dtype, ww, nb, cost.ctypes.data,
                                               order.ctypes.data, status.ctypes.data, None) == EINVAL
        assert L.tspgpu_solve_paths_cities(None, cities, ww, nb, tspgpu._dp(cost), tspgpu._ip(order),
                                           tspgpu._ip(status)) == EINVAL
        assert L.tspgpu_solve_paths_cities_device(None, addr, ww, nb, cost.ctypes.data, order.ctypes.data,
                                                  status.ctypes.data, None) == EINVAL
    for LL, m, mp in ((12, 7, 8), (1, 7, 8), (12, 1, 8), (12, 19, 8), (12, 7, 0)):
        assert L.tspgpu_refine_path(None, cities, LL, m, mp, out, ctypes.byref(st)) == EINVAL
        assert L.tspgpu_refine_path_device(None, addr, LL, m, mp, ctypes.byref(st), None) == EINVAL
    assert (dist == 7.0).all() and (cost == 7.0).all() and (order == 7).all() and (status == 7).all()
    assert st.passes == 7 and all(c.id == 0 for c in out)


def test_path_length_on_the_host():
    L = tspgpu.lib()
    out = ctypes.c_double(7.0)
    cities, _, _ = tspgpu.cities_array([[(0, 0.0, 0.0), (1, 3.0, 4.0)]])
    assert L.tspgpu_path_length(None, 2, ctypes.byref(out)) == EINVAL
    assert L.tspgpu_path_length(cities, 2, None) == EINVAL
    assert L.tspgpu_path_length(cities, 0, ctypes.byref(out)) == EINVAL and out.value == 7.0
    assert tspgpu.path_length([(0, 0.0, 0.0), (1, 3.0, 4.0)]) == 5.0
    assert tspgpu.path_length([(0, 1.5, 2.5)]) == 0.0
    for path in (R.scrambled(300, 1), R.shuffled_line(100, 2), R.lattice_scrambled(100, 3)):
        assert struct.pack("<d", tspgpu.path_length(path)) == struct.pack("<d", R.path_length(path))


def test_binding_has_the_methods():
    for name in ("solve_paths", "solve_paths_device", "solve_paths_cities", "solve_paths_cities_device", "refine_path",
                 "refine_path_device"):
        assert callable(getattr(tspgpu.Context, name, None)), name
    sig = inspect.signature(tspgpu.Context.refine_path).parameters
    assert sig["interior"].default == 15 and sig["max_passes"].default == 8
    for name in ("pipeline_cities", "pipeline_cities_ragged"):
        assert inspect.signature(getattr(tspgpu.Context, name)).parameters["refine"].default == 0
    assert ctypes.sizeof(tspgpu.RefineStats) == 64
