"""Ragged batches, the part that needs no GPU: the two entries are exported, a
NULL context is refused before any HIP call and nothing is written, and the
binding carries the methods.  (tests/test_abi.py checks the header side: every
declared symbol is exported.)"""
import ctypes
import errno

import numpy as np

import tspgpu

NAMES = {"tspgpu_solve_ragged", "tspgpu_solve_ragged_device"}


def test_symbols_exported():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NAMES)
    assert NAMES <= set(tspgpu.EXPORTED_SYMBOLS)


def test_null_context_refused_without_a_device():
    L = tspgpu.lib()
    d = np.ones(25 + 9, dtype=np.float64)
    off = np.array([0, 25], dtype=np.int64)
    n = np.array([5, 3], dtype=np.int32)
    cost = np.full(2, 7.0)
    tour = np.full((2, 6), 7, dtype=np.int32)
    status = np.full(2, 7, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    i64p = ctypes.POINTER(ctypes.c_int64)
    for dtype in (tspgpu.F64, tspgpu.I32, 5):
        rc = L.tspgpu_solve_ragged(None, d.ctypes.data, dtype, off.ctypes.data_as(i64p), n.ctypes.data_as(ip), 2,
                                   cost.ctypes.data, tour.ctypes.data_as(ip), 6, status.ctypes.data_as(ip))
        assert rc == -errno.EINVAL
        rc = L.tspgpu_solve_ragged_device(None, d.ctypes.data, dtype, off.ctypes.data_as(i64p), n.ctypes.data_as(ip),
                                          2, cost.ctypes.data, tour.ctypes.data, 6, status.ctypes.data, None)
        assert rc == -errno.EINVAL
    # (also with nothing to do: the context is checked first)
    assert L.tspgpu_solve_ragged(None, None, tspgpu.F64, None, None, 0, None, None, 1, None) == -errno.EINVAL
    assert (cost == 7.0).all() and (tour == 7).all() and (status == 7).all()


def test_binding_has_the_methods():
    assert callable(getattr(tspgpu.Context, "solve_ragged", None))
    assert callable(getattr(tspgpu.Context, "solve_ragged_device", None))
    assert callable(getattr(tspgpu.Context, "solve_ragged_flat", None))
