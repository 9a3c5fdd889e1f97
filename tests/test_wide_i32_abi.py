"""K1-wide on int32 distances, the part that needs no GPU: the two entries
are exported, the int32 entry refuses NULL arguments before any HIP call, and
the binding carries the methods.  (tests/test_abi.py checks the header side:
every declared symbol is exported.)"""
import ctypes
import errno

import numpy as np

import tspgpu


def test_symbols_exported():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert hasattr(L, "tspgpu_solve_instance_i32") and hasattr(L, "tspgpu_wide_last_dtype")
    assert {"tspgpu_solve_instance_i32", "tspgpu_wide_last_dtype"} <= set(tspgpu.EXPORTED_SYMBOLS)


def test_null_arguments_refused_without_a_device():
    L = tspgpu.lib()
    d = np.zeros((5, 5), dtype=np.int32)
    cost, ms = ctypes.c_int32(7), ctypes.c_double()
    tour = np.zeros(6, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = L.tspgpu_solve_instance_i32(None, d.ctypes.data_as(ip), 5, ctypes.byref(cost), tour.ctypes.data_as(ip),
                                     ctypes.byref(ms))
    assert rc == -errno.EINVAL and cost.value == 7
    assert L.tspgpu_wide_last_dtype(None) == -1


def test_binding_has_the_methods():
    assert callable(getattr(tspgpu.Context, "solve_instance_i32", None))
    assert callable(getattr(tspgpu.Context, "wide_last_dtype", None))
