"""Or-opt with a neighbour grid, the part that needs no GPU: the entry points are
exported, the argument errors that are decided before any device work are
refused and nothing is written, and the binding carries the methods.
(tests/test_abi.py checks the header side: every declared symbol is exported.)"""
import ctypes
import errno
import inspect

import tspgpu

NAMES = {"tspgpu_or_opt_path", "tspgpu_or_opt_path_device"}
EINVAL = -errno.EINVAL


def test_symbols_exported():
    L = ctypes.CDLL(tspgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NAMES)
    assert NAMES <= set(tspgpu.EXPORTED_SYMBOLS)


def test_null_context_and_bad_arguments_refused_without_a_device():
    L = tspgpu.lib()
    cities, _, _ = tspgpu.cities_array([[(i, float(i), 2.0 * i) for i in range(12)]])
    out = (tspgpu.City * 12)()
    st = tspgpu.OrOptStats(passes=7, gain=7.0)
    addr = ctypes.addressof(cities)
    # (the context is checked first, also with good arguments and with nothing to do)
    for LL, ring, seg, mp in ((12, 2, 3, 1000), (3, 2, 3, 1000), (0, 2, 3, 8), (-1, 2, 3, 8), (12, 0, 3, 8),
                              (12, 5, 3, 8), (12, 2, 0, 8), (12, 2, 4, 8), (12, 2, 3, 0)):
        assert L.tspgpu_or_opt_path(None, cities, LL, ring, seg, mp, out, ctypes.byref(st)) == EINVAL
        assert L.tspgpu_or_opt_path_device(None, addr, LL, ring, seg, mp, ctypes.byref(st), None) == EINVAL
    assert L.tspgpu_or_opt_path(None, None, 12, 2, 3, 8, out, None) == EINVAL
    assert st.passes == 7 and st.gain == 7.0 and st.moves == 0 and all(c.id == 0 for c in out)
    assert [cities[i].id for i in range(12)] == list(range(12))


def test_binding_has_the_methods():
    for name in ("or_opt_path", "or_opt_path_device"):
        assert callable(getattr(tspgpu.Context, name, None)), name
        sig = inspect.signature(getattr(tspgpu.Context, name)).parameters
        assert sig["ring"].default == 2 and sig["max_seg"].default == 3 and sig["max_passes"].default == 1000
    for name in ("pipeline_cities", "pipeline_cities_ragged"):
        sig = inspect.signature(getattr(tspgpu.Context, name)).parameters
        assert sig["or_opt"].default == 0 and sig["two_opt"].default == 0 and sig["refine"].default == 0
    # the same fields as tspgpu_two_opt_stats
    assert ctypes.sizeof(tspgpu.OrOptStats) == ctypes.sizeof(tspgpu.TwoOptStats) == 64
    assert [f for f, _ in tspgpu.OrOptStats._fields_] == ["passes", "candidates", "moves", "gain", "grid_ms",
                                                          "search_ms", "select_ms", "apply_ms"]
    assert [(f, getattr(tspgpu.OrOptStats, f).offset) for f, _ in tspgpu.OrOptStats._fields_] == [
        (f, getattr(tspgpu.TwoOptStats, f).offset) for f, _ in tspgpu.TwoOptStats._fields_]
