"""Distances on the device, the part that needs no GPU: the entry points are
exported, the argument errors that are decided before any device work are
refused and nothing is written, and the binding carries the methods.
(tests/test_abi.py checks the header side: every declared symbol is exported.)"""
import ctypes
import errno

import numpy as np

import tspgpu

NAMES = {"tspgpu_distance_matrix_device", "tspgpu_solve_cities_device", "tspgpu_solve_cities_upload",
         "tspgpu_cities_last_fixups", "tspgpu_cities_last_phase_ms"}
EINVAL = -errno.EINVAL


def test_symbols_exported():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NAMES)
    assert NAMES <= set(tspgpu.EXPORTED_SYMBOLS)


def test_null_context_refused_without_a_device():
    L = tspgpu.lib()
    cities, n, B = tspgpu.cities_array([[(i, float(i), 2.0 * i) for i in range(5)]] * 2)
    dist = np.full((2, 5, 5), 7.0)
    cost = np.full(2, 7.0)
    tour = np.full((2, 6), 7, dtype=np.int32)
    status = np.full(2, 7, dtype=np.int32)
    addr = ctypes.addressof(cities)
    for nn, nb in ((5, 2), (1, 2), (0, 2), (21, 2), (5, -1), (5, 0)):
        # (the context is checked first, also with nothing to do)
        assert L.tspgpu_distance_matrix_device(None, addr, nn, nb, dist.ctypes.data, None) == EINVAL
        assert L.tspgpu_solve_cities_device(None, addr, nn, nb, cost.ctypes.data, tour.ctypes.data,
                                            status.ctypes.data, None) == EINVAL
        assert L.tspgpu_solve_cities_upload(None, cities, nn, nb, tspgpu._dp(cost), tspgpu._ip(tour)) == EINVAL
    assert L.tspgpu_cities_last_fixups(None, None, None, None) == EINVAL
    assert L.tspgpu_cities_last_phase_ms(None, None, None) == EINVAL
    assert (dist == 7.0).all() and (cost == 7.0).all() and (tour == 7).all() and (status == 7).all()


def test_binding_has_the_methods():
    for name in ("distance_matrix_device", "solve_cities_device", "solve_cities", "cities_last_fixups",
                 "cities_last_phase_ms"):
        assert callable(getattr(tspgpu.Context, name, None)), name
    import inspect

    assert inspect.signature(tspgpu.Context.solve_cities).parameters["device_dist"].default is False
    assert tspgpu.CITY_DTYPE.itemsize == ctypes.sizeof(tspgpu.City) == 24
    assert tspgpu.lib().tspgpu_tuning_set(b"DIST_FIX_CAP", 64.0) == 0
    assert tspgpu.lib().tspgpu_tuning_clear(b"DIST_FIX_CAP") == 0
