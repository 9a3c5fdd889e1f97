"""ctypes binding of libtspgpu (include/tspgpu.h) for tests and bench.py.

This is the same C ABI a ctypes user of the reference's block solver would
bind.  It never falls back to CPU code: if lib/libtspgpu.so
is missing or no HIP device is present, the calls raise.
"""
from __future__ import annotations

import ctypes
import errno
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# TSPGPU_LIB: another build of the same ABI (development A/B experiments)
LIB_PATH = os.environ.get("TSPGPU_LIB") or os.path.join(PKG_DIR, "lib", "libtspgpu.so")
HOST_LIB_PATH = os.path.join(PKG_DIR, "lib", "libtsphost.so")
TSP_BIN = os.path.join(PKG_DIR, "bin", "tsp")

EXPORTED_SYMBOLS = (
    "tspgpu_version", "tspgpu_strerror", "tspgpu_tour_length", "tspgpu_distance_matrix", "tspgpu_validate",
    "tspgpu_ctx_create", "tspgpu_ctx_destroy", "tspgpu_solve_blocks", "tspgpu_solve_cities",
    "tspgpu_solve_blocks_device", "tspgpu_solve", "tspgpu_last_grid", "tspgpu_relaxations_per_block",
    "tspgpu_table_bytes_per_block", "tspgpu_device_alloc", "tspgpu_device_free", "tspgpu_memcpy_htod",
    "tspgpu_memcpy_dtoh", "tspgpu_stream", "tspgpu_synchronize", "tspgpu_timer_start", "tspgpu_timer_stop",
    "tspgpu_device_info", "tspgpu_last_variant", "tspgpu_k1_split_timing", "tspgpu_k1_last_split_ms", "tspgpu_device_count", "tspgpu_stream_create",
    "tspgpu_stream_destroy", "tspgpu_stream_synchronize",
    # K2
    "tspgpu_search_solve", "tspgpu_search_enumerate", "tspgpu_search_create", "tspgpu_search_create_ex",
    "tspgpu_search_destroy", "tspgpu_search_info",
    "tspgpu_search_set_bound", "tspgpu_search_start", "tspgpu_search_step", "tspgpu_search_run_all",
    "tspgpu_search_timing", "tspgpu_search_incumbent_device", "tspgpu_search_chain", "tspgpu_search_tie_slot",
    "tspgpu_search_counters", "tspgpu_search_reset_records", "tspgpu_search_records", "tspgpu_heuristic_tour",
    "tspgpu_heuristic_tour_starts",
    "tspgpu_select_tour", "tspgpu_tie_tour", "tspgpu_tie_tour_gpu", "tspgpu_tie_tour_records", "tspgpu_tie_key",
    # K3
    "tspgpu_merge", "tspgpu_reduce",
    # K3 with the merged tour, and from K1's device outputs (no visit to the host in between)
    "tspgpu_reduce_path", "tspgpu_reduce_device", "tspgpu_reduce_device_last_ms", "tspgpu_pipeline_cities",
    # K1-wide
    "tspgpu_solve_instance", "tspgpu_solve_instance_i32", "tspgpu_wide_last_dtype",
    # K1 on integer distances
    "tspgpu_validate_i32", "tspgpu_solve_blocks_i32", "tspgpu_solve_blocks_i32_device",
    # ragged batches (blocks of different sizes, validated per block on the device)
    "tspgpu_solve_ragged", "tspgpu_solve_ragged_device",
    # distances on the device (cities in device memory, the host's pow on the flagged squares only)
    "tspgpu_distance_matrix_device", "tspgpu_solve_cities_device", "tspgpu_solve_cities_upload",
    "tspgpu_cities_last_fixups", "tspgpu_cities_last_phase_ms",
    # ragged blocks end to end: packed cities of different block sizes -> distances, K1, K3, the merged tour
    "tspgpu_distance_matrix_ragged_device", "tspgpu_solve_cities_ragged_device", "tspgpu_solve_cities_ragged",
    "tspgpu_reduce_ragged_device", "tspgpu_reduce_ragged", "tspgpu_pipeline_cities_ragged",
    # fixed-end shortest paths (K1 on the folded matrix) and the window refinement of a tour on the device
    "tspgpu_solve_paths", "tspgpu_solve_paths_device", "tspgpu_solve_paths_cities", "tspgpu_solve_paths_cities_device",
    "tspgpu_refine_path", "tspgpu_refine_path_device", "tspgpu_path_length",
    # 2-opt with a neighbour grid on a path, the stage in front of the window refinement
    "tspgpu_two_opt_path", "tspgpu_two_opt_path_device",
    # Or-opt (segment insertion) on the same grid, between 2-opt and the window refinement
    "tspgpu_or_opt_path", "tspgpu_or_opt_path_device",
    # tuning / test knobs
    "tspgpu_tuning_set", "tspgpu_tuning_clear",
)

F64, I32 = 0, 1
SEARCH_DEVICE_BOUND, SEARCH_EXHAUSTIVE = 1, 2  # tspgpu_search_create_ex flags
SEARCH_MAX_CITIES = 32
MAX_CITIES = 20  # TSPGPU_MAX_CITIES: the batched K1 (extension sizes above the reference's 16)


class TourRecord(ctypes.Structure):
    """tspgpu_tour_record: cost bits + inner cities t1..tN."""
    _fields_ = [("cost", ctypes.c_uint64), ("city", ctypes.c_uint8 * 32)]


class SearchStats(ctypes.Structure):
    _fields_ = [("nodes", ctypes.c_uint64), ("records", ctypes.c_uint64), ("optimal_tours", ctypes.c_uint64),
                ("items", ctypes.c_uint64), ("depth", ctypes.c_int), ("phases", ctypes.c_int),
                ("fallback", ctypes.c_int), ("rounds", ctypes.c_int), ("kernel_ms", ctypes.c_double),
                ("lane_steps", ctypes.c_uint64), ("active_steps", ctypes.c_uint64), ("item_loads", ctypes.c_uint64),
                ("tie", ctypes.c_int), ("tie_checked", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TieSlot(ctypes.Structure):
    """tspgpu_tie_slot: a shard's least tie key at one cost."""
    _fields_ = [("w0", ctypes.c_uint64), ("w1", ctypes.c_uint64), ("found", ctypes.c_int),
                ("overflow", ctypes.c_int)]


class RefineStats(ctypes.Structure):
    """tspgpu_refine_stats: what a window refinement did, and its device times."""
    _fields_ = [("passes", ctypes.c_int), ("windows", ctypes.c_int64), ("replaced", ctypes.c_int64),
                ("skipped", ctypes.c_int64), ("gain", ctypes.c_double), ("build_ms", ctypes.c_double),
                ("k1_ms", ctypes.c_double), ("fold_apply_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TwoOptStats(ctypes.Structure):
    """tspgpu_two_opt_stats: what a 2-opt call did, and its phase times."""
    _fields_ = [("passes", ctypes.c_int), ("candidates", ctypes.c_int64), ("moves", ctypes.c_int64),
                ("gain", ctypes.c_double), ("grid_ms", ctypes.c_double), ("search_ms", ctypes.c_double),
                ("select_ms", ctypes.c_double), ("apply_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OrOptStats(ctypes.Structure):
    """tspgpu_or_opt_stats: what an Or-opt call did, and its phase times."""
    _fields_ = list(TwoOptStats._fields_)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


LEVEL_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)


class City(ctypes.Structure):
    """tspgpu_city == the reference's City (assignment2.h:13-18)."""
    _fields_ = [("id", ctypes.c_int32), ("x", ctypes.c_double), ("y", ctypes.c_double)]


# the same 24 bytes for numpy: np.frombuffer(city_array, CITY_DTYPE), Context.upload(...)
CITY_DTYPE = np.dtype([("id", "<i4"), ("x", "<f8"), ("y", "<f8")], align=True)
assert CITY_DTYPE.itemsize == ctypes.sizeof(City) == 24


class Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("strict", ctypes.c_int), ("slots", ctypes.c_int),
                ("reserved", ctypes.c_int * 5)]


class TspGpuError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {lib().tspgpu_strerror(code).decode()} ({code})")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not built (make -C tsp-mpi-reduction_amd)")
        L = ctypes.CDLL(LIB_PATH)
        dp = ctypes.POINTER(ctypes.c_double)
        ip = ctypes.POINTER(ctypes.c_int32)
        vp = ctypes.c_void_p
        L.tspgpu_version.restype = ctypes.c_int
        L.tspgpu_strerror.argtypes = [ctypes.c_int]
        L.tspgpu_strerror.restype = ctypes.c_char_p
        L.tspgpu_tour_length.argtypes = [ctypes.c_int]
        L.tspgpu_distance_matrix.argtypes = [ctypes.POINTER(City), ctypes.c_int, ctypes.c_int, dp]
        L.tspgpu_validate.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.tspgpu_ctx_create.argtypes = [ctypes.POINTER(Opts), ctypes.POINTER(vp)]
        L.tspgpu_ctx_destroy.argtypes = [vp]
        L.tspgpu_solve_blocks.argtypes = [vp, dp, ctypes.c_int, ctypes.c_int, dp, ip]
        L.tspgpu_solve_cities.argtypes = [vp, ctypes.POINTER(City), ctypes.c_int, ctypes.c_int, dp, ip]
        L.tspgpu_solve_blocks_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
        L.tspgpu_validate_i32.argtypes = [ip, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.tspgpu_solve_blocks_i32.argtypes = [vp, ip, ctypes.c_int, ctypes.c_int, ip, ip]
        L.tspgpu_solve_blocks_i32_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
        i64p = ctypes.POINTER(ctypes.c_int64)
        L.tspgpu_solve_ragged.argtypes = [vp, vp, ctypes.c_int, i64p, ip, ctypes.c_int, vp, ip, ctypes.c_int, ip]
        L.tspgpu_solve_ragged_device.argtypes = [vp, vp, ctypes.c_int, i64p, ip, ctypes.c_int, vp, vp, ctypes.c_int,
                                                 vp, vp]
        L.tspgpu_distance_matrix_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
        L.tspgpu_solve_cities_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        L.tspgpu_solve_cities_upload.argtypes = [vp, ctypes.POINTER(City), ctypes.c_int, ctypes.c_int, dp, ip]
        L.tspgpu_cities_last_fixups.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.POINTER(ctypes.c_int)]
        L.tspgpu_cities_last_phase_ms.argtypes = [vp, dp, dp]
        L.tspgpu_solve.argtypes = [dp, ctypes.c_int, ctypes.c_int, dp, ip, ctypes.POINTER(Opts)]
        L.tspgpu_last_grid.argtypes = [vp]
        L.tspgpu_last_variant.argtypes = [vp]
        L.tspgpu_k1_split_timing.argtypes = [vp, ctypes.c_int]
        L.tspgpu_k1_last_split_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.tspgpu_device_count.argtypes = []
        L.tspgpu_relaxations_per_block.argtypes = [ctypes.c_int]
        L.tspgpu_relaxations_per_block.restype = ctypes.c_double
        L.tspgpu_table_bytes_per_block.argtypes = [ctypes.c_int]
        L.tspgpu_table_bytes_per_block.restype = ctypes.c_double
        L.tspgpu_device_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.tspgpu_device_free.argtypes = [vp, vp]
        L.tspgpu_memcpy_htod.argtypes = [vp, vp, vp, ctypes.c_size_t]
        L.tspgpu_memcpy_dtoh.argtypes = [vp, vp, vp, ctypes.c_size_t]
        L.tspgpu_stream.argtypes = [vp]
        L.tspgpu_stream.restype = vp
        L.tspgpu_synchronize.argtypes = [vp]
        L.tspgpu_stream_create.argtypes = [vp, ctypes.POINTER(vp)]
        L.tspgpu_stream_destroy.argtypes = [vp, vp]
        L.tspgpu_stream_synchronize.argtypes = [vp, vp]
        L.tspgpu_timer_start.argtypes = [vp]
        L.tspgpu_timer_stop.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.tspgpu_device_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.tspgpu_search_solve.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, dp, ip, ctypes.POINTER(SearchStats)]
        L.tspgpu_search_enumerate.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, dp, ip, ctypes.POINTER(SearchStats)]
        L.tspgpu_search_create.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(vp)]
        L.tspgpu_search_create_ex.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.tspgpu_search_destroy.argtypes = [vp]
        L.tspgpu_search_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int), u64p, u64p]
        L.tspgpu_search_set_bound.argtypes = [vp, ctypes.c_double]
        L.tspgpu_search_start.argtypes = [vp]
        L.tspgpu_search_step.argtypes = [vp, u64p]
        L.tspgpu_search_run_all.argtypes = [vp]
        L.tspgpu_search_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
        L.tspgpu_search_incumbent_device.argtypes = [vp]
        L.tspgpu_search_incumbent_device.restype = vp
        L.tspgpu_search_counters.argtypes = [vp, u64p, u64p, u64p]
        L.tspgpu_search_chain.argtypes = [vp, ctypes.c_int, LEVEL_HOOK, vp, ctypes.POINTER(ctypes.c_int)]
        L.tspgpu_search_tie_slot.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(TieSlot)]
        L.tspgpu_search_reset_records.argtypes = [vp, ctypes.c_uint]
        L.tspgpu_search_records.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(TourRecord), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_int)]
        L.tspgpu_heuristic_tour.argtypes = [vp, ctypes.c_int, ctypes.c_int, dp, ip]
        L.tspgpu_heuristic_tour_starts.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, ip]
        L.tspgpu_select_tour.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(TourRecord), ctypes.c_int,
                                         ctypes.c_uint64, ip]
        L.tspgpu_tie_tour.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                      ip]
        L.tspgpu_tuning_set.argtypes = [ctypes.c_char_p, ctypes.c_double]
        L.tspgpu_tuning_clear.argtypes = [ctypes.c_char_p]
        L.tspgpu_tie_tour_gpu.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                          ctypes.c_uint64, ip]
        L.tspgpu_tie_tour_records.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                              ctypes.c_uint64, ctypes.POINTER(TourRecord), ctypes.c_int, ip]
        L.tspgpu_tie_key.argtypes = [ctypes.c_int, ip, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        cp = ctypes.POINTER(City)
        L.tspgpu_solve_instance.argtypes = [vp, dp, ctypes.c_int, dp, ip, dp]
        L.tspgpu_solve_instance_i32.argtypes = [vp, ip, ctypes.c_int, ip, ip, dp]
        L.tspgpu_wide_last_dtype.argtypes = [vp]
        L.tspgpu_merge.argtypes = [vp, cp, ctypes.c_int, ctypes.c_double, cp, ctypes.c_int, ctypes.c_double, cp, dp]
        L.tspgpu_reduce.argtypes = [vp, cp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int, dp, ctypes.c_char_p,
                                    ctypes.c_int]
        intp = ctypes.POINTER(ctypes.c_int)
        L.tspgpu_reduce_path.argtypes = [vp, cp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int, dp, cp, ctypes.c_int,
                                         intp, ctypes.c_char_p, ctypes.c_int]
        L.tspgpu_reduce_device.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, vp,
                                           ctypes.c_int, intp, ctypes.c_char_p, ctypes.c_int, vp]
        L.tspgpu_reduce_device_last_ms.argtypes = [vp, dp]
        L.tspgpu_pipeline_cities.argtypes = [vp, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, cp, ctypes.c_int,
                                             intp, ctypes.c_char_p, ctypes.c_int]
        L.tspgpu_distance_matrix_ragged_device.argtypes = [vp, vp, ip, ctypes.c_int, vp, vp]
        L.tspgpu_solve_cities_ragged_device.argtypes = [vp, vp, ip, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp]
        L.tspgpu_solve_cities_ragged.argtypes = [vp, cp, ip, ctypes.c_int, dp, ip, ctypes.c_int, ip]
        L.tspgpu_reduce_ragged_device.argtypes = [vp, vp, ip, vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, dp,
                                                  vp, ctypes.c_int, intp, ctypes.c_char_p, ctypes.c_int, vp]
        L.tspgpu_reduce_ragged.argtypes = [vp, cp, ip, dp, ctypes.c_int, ctypes.c_int, dp, cp, ctypes.c_int, intp,
                                           ctypes.c_char_p, ctypes.c_int]
        L.tspgpu_pipeline_cities_ragged.argtypes = [vp, cp, ip, ctypes.c_int, ctypes.c_int, dp, cp, ctypes.c_int,
                                                    intp, ctypes.c_char_p, ctypes.c_int]
        L.tspgpu_solve_paths.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ip, ip]
        L.tspgpu_solve_paths_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        L.tspgpu_solve_paths_cities.argtypes = [vp, cp, ctypes.c_int, ctypes.c_int, dp, ip, ip]
        L.tspgpu_solve_paths_cities_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        rsp = ctypes.POINTER(RefineStats)
        L.tspgpu_refine_path.argtypes = [vp, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, cp, rsp]
        L.tspgpu_refine_path_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, rsp, vp]
        L.tspgpu_path_length.argtypes = [cp, ctypes.c_int, dp]
        tsp = ctypes.POINTER(TwoOptStats)
        L.tspgpu_two_opt_path.argtypes = [vp, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, cp, tsp]
        L.tspgpu_two_opt_path_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, tsp, vp]
        osp = ctypes.POINTER(OrOptStats)
        L.tspgpu_or_opt_path.argtypes = [vp, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, cp, osp]
        L.tspgpu_or_opt_path_device.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, osp, vp]
        _lib = L
    return _lib


def tune(name: str, value) -> None:
    """Set a tuning / test knob (tspgpu_tuning_set; include/tspgpu.h
    "Tuning"): process-wide, read where the knob is used (K1 knobs at
    Context creation, K2 knobs at search creation)."""
    rc = lib().tspgpu_tuning_set(name.encode(), float(value))
    if rc:
        raise TspGpuError(rc, f"tspgpu_tuning_set({name})")


def tune_from_environ() -> None:
    """Development tools only (tools/*.py): every TSPGPU_<KNOB>=value of this
    process's environment as tune(KNOB, value).  The library itself reads no
    environment variable; neither the tests nor bench.py call this."""
    for k, v in os.environ.items():
        if k.startswith("TSPGPU_") and k != "TSPGPU_LIB":
            tune(k[len("TSPGPU_"):], float(v))


def untune(name: str | None = None) -> None:
    """Back to the default (None: every knob)."""
    rc = lib().tspgpu_tuning_clear(name.encode() if name else None)
    if rc:
        raise TspGpuError(rc, f"tspgpu_tuning_clear({name})")


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def device_count() -> int:
    """Visible HIP devices (initialises HIP in this process)."""
    return lib().tspgpu_device_count()


def tour_length(n: int) -> int:
    return lib().tspgpu_tour_length(n)


def relaxations_per_block(n: int) -> float:
    return lib().tspgpu_relaxations_per_block(n)


def table_bytes_per_block(n: int) -> float:
    return lib().tspgpu_table_bytes_per_block(n)


def cities_array(blocks):
    """blocks: list of blocks, each a list of (id, x, y) -> (ctypes City array, n, B)."""
    B = len(blocks)
    n = len(blocks[0]) if B else 0
    arr = (City * max(1, B * n))()
    for b, blk in enumerate(blocks):
        assert len(blk) == n
        for j, (cid, x, y) in enumerate(blk):
            c = arr[b * n + j]
            c.id, c.x, c.y = int(cid), float(x), float(y)
    return arr, n, B


def cities_array_ragged(blocks):
    """blocks of different sizes, each a list of (id, x, y) -> (ctypes City
    array of the packed cities in block order, n (B,) int32)."""
    ns = np.array([len(blk) for blk in blocks], dtype=np.int32)
    arr = (City * max(1, int(ns.sum())))()
    k = 0
    for blk in blocks:
        for cid, x, y in blk:
            c = arr[k]
            c.id, c.x, c.y = int(cid), float(x), float(y)
            k += 1
    return arr, ns


def distance_matrix(blocks) -> np.ndarray:
    """Host libm distances, bit-exact with computeDistanceMatrix (assignment2.h:184-200)."""
    arr, n, B = cities_array(blocks)
    d = np.zeros((B, n, n), dtype=np.float64)
    rc = lib().tspgpu_distance_matrix(arr, n, B, _dp(d))
    if rc:
        raise TspGpuError(rc, "tspgpu_distance_matrix")
    return d


def distance_matrix_array(arr, n: int, B: int) -> np.ndarray:
    """Same, from a ctypes City array of B*n cities."""
    d = np.zeros((B, n, n), dtype=np.float64)
    rc = lib().tspgpu_distance_matrix(arr, n, B, _dp(d))
    if rc:
        raise TspGpuError(rc, "tspgpu_distance_matrix")
    return d


def path_length(path) -> float:
    """tspgpu_path_length: the left fold, in path order, of the reference's
    distance() on consecutive cities of a path (list of (id, x, y)); host
    glibc.  The yardstick for refine_path's before and after."""
    arr, L, _ = cities_array([path])
    out = ctypes.c_double()
    rc = lib().tspgpu_path_length(arr, L, ctypes.byref(out))
    if rc:
        raise TspGpuError(rc, "tspgpu_path_length")
    return out.value


def validate(dist: np.ndarray, strict: bool = False) -> int:
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    B, n, _ = dist.shape
    return lib().tspgpu_validate(_dp(dist), n, B, int(strict))


def validate_i32(dist: np.ndarray, strict: bool = False) -> int:
    dist = np.ascontiguousarray(dist, dtype=np.int32)
    B, n, _ = dist.shape
    return lib().tspgpu_validate_i32(_ip(dist), n, B, int(strict))


class Context:
    """Owns a tspgpu_ctx (device memory, stream) on one HIP device."""

    def __init__(self, device: int = -1, strict: bool = False, slots: int = 0):
        o = Opts(device, int(strict), slots)
        h = ctypes.c_void_p()
        rc = lib().tspgpu_ctx_create(ctypes.byref(o), ctypes.byref(h))
        if rc:
            raise TspGpuError(rc, "tspgpu_ctx_create")
        self.handle = h

    def close(self):
        # (destroy order is free in the C ABI: live searches keep the
        # context, the last Search.close releases it — include/tspgpu.h)
        if self.handle:
            lib().tspgpu_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def solve_blocks(self, dist: np.ndarray):
        """dist: (B, n, n) float64 -> (costs (B,), tours (B, n+1) int32, -1 padded)."""
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        B, n, _ = dist.shape
        cost = np.zeros(B, dtype=np.float64)
        tour = np.full((B, n + 1), -1, dtype=np.int32)
        rc = lib().tspgpu_solve_blocks(self.handle, _dp(dist), n, B, _dp(cost), _ip(tour))
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_blocks")
        return cost, tour

    def solve_blocks_i32(self, dist: np.ndarray):
        """dist: (B, n, n) int32 -> (costs (B,) int32, tours (B, n+1) int32, -1 padded)."""
        dist = np.ascontiguousarray(dist, dtype=np.int32)
        B, n, _ = dist.shape
        cost = np.zeros(B, dtype=np.int32)
        tour = np.full((B, n + 1), -1, dtype=np.int32)
        rc = lib().tspgpu_solve_blocks_i32(self.handle, _ip(dist), n, B, _ip(cost), _ip(tour))
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_blocks_i32")
        return cost, tour

    def solve_device_i32(self, d_dist_ptr: int, n: int, nblocks: int, d_cost_ptr: int, d_tour_ptr: int,
                         stream_ptr: int = 0):
        rc = lib().tspgpu_solve_blocks_i32_device(self.handle, d_dist_ptr, n, nblocks, d_cost_ptr, d_tour_ptr,
                                                  stream_ptr)
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_blocks_i32_device")

    def solve_cities(self, blocks, device_dist: bool = False):
        """blocks: lists of (id, x, y), or a (ctypes City array, n, B) triple ->
        (costs, tours).  device_dist: upload the cities and build the matrices
        on the device (tspgpu_solve_cities_upload) instead of on the host."""
        arr, n, B = blocks if isinstance(blocks, tuple) else cities_array(blocks)
        cost = np.zeros(B, dtype=np.float64)
        tour = np.full((B, n + 1), -1, dtype=np.int32)
        fn, what = ((lib().tspgpu_solve_cities_upload, "tspgpu_solve_cities_upload") if device_dist else
                    (lib().tspgpu_solve_cities, "tspgpu_solve_cities"))
        rc = fn(self.handle, arr, n, B, _dp(cost), _ip(tour))
        if rc:
            raise TspGpuError(rc, what)
        return cost, tour

    def distance_matrix_device(self, d_cities_ptr: int, n: int, nblocks: int, d_dist_ptr: int, stream_ptr: int = 0):
        """tspgpu_distance_matrix_device: nblocks*n City structs at d_cities_ptr
        -> nblocks*n*n float64 at d_dist_ptr, the bits of distance_matrix().
        Synchronises the stream once; the last kernels are left running."""
        rc = lib().tspgpu_distance_matrix_device(self.handle, d_cities_ptr, n, nblocks, d_dist_ptr, stream_ptr)
        if rc:
            raise TspGpuError(rc, "tspgpu_distance_matrix_device")

    def solve_cities_device(self, d_cities_ptr: int, n: int, nblocks: int, d_cost_ptr: int, d_tour_ptr: int,
                            d_status_ptr: int, stream_ptr: int = 0):
        """tspgpu_solve_cities_device: cities on the device -> cost (B float64),
        tours (B x (n+1) int32) and status (B int32) on the device, under the
        ragged contract (a bad block: its status, NaN, a row of -1)."""
        rc = lib().tspgpu_solve_cities_device(self.handle, d_cities_ptr, n, nblocks, d_cost_ptr, d_tour_ptr,
                                              d_status_ptr, stream_ptr)
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_cities_device")

    def cities_last_fixups(self):
        """(squares, flagged, build_passes) of this context's last device distance build."""
        sq, fl, ps = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        self._check(lib().tspgpu_cities_last_fixups(self.handle, ctypes.byref(sq), ctypes.byref(fl),
                                                    ctypes.byref(ps)), "tspgpu_cities_last_fixups")
        return sq.value, fl.value, ps.value

    def cities_last_phase_ms(self):
        """(build_ms, pow_ms): host wall time of the last build's kernel + list
        copy + synchronisation, and of its pow calls."""
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(lib().tspgpu_cities_last_phase_ms(self.handle, ctypes.byref(a), ctypes.byref(b)),
                    "tspgpu_cities_last_phase_ms")
        return a.value, b.value

    def solve_device(self, d_dist_ptr: int, n: int, nblocks: int, d_cost_ptr: int, d_tour_ptr: int,
                     stream_ptr: int = 0):
        rc = lib().tspgpu_solve_blocks_device(self.handle, d_dist_ptr, n, nblocks, d_cost_ptr, d_tour_ptr,
                                              stream_ptr)
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_blocks_device")

    def solve_ragged(self, mats, tour_stride: int | None = None):
        """Blocks of different sizes in one call (tspgpu_solve_ragged), each
        validated on the device.  mats: a sequence of square arrays, all
        float64 (or convertible) or all int32 -> (cost (B,) float64 / int32,
        tours (B, max n + 1) int32 padded with -1, status (B,) int32).  Status
        0: cost and tour as solve_blocks / solve_blocks_i32 give them; else a
        negative errno, cost NaN / -1 and the tour row all -1."""
        mats = [np.asarray(m) for m in mats]
        integer = bool(mats) and all(np.issubdtype(m.dtype, np.integer) for m in mats)
        dt = np.int32 if integer else np.float64
        for m in mats:
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError(f"solve_ragged: a block of shape {m.shape} is not square")
        ns = np.array([m.shape[0] for m in mats], dtype=np.int32)
        sizes = ns.astype(np.int64) ** 2
        offset = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64) if len(mats) else np.zeros(0, np.int64)
        flat = np.concatenate([np.ascontiguousarray(m, dtype=dt).ravel() for m in mats]) if mats else np.zeros(0, dt)
        return self.solve_ragged_flat(flat, offset, ns, tour_stride)

    def solve_ragged_flat(self, dist: np.ndarray, offset, n, tour_stride: int | None = None, out=None):
        """tspgpu_solve_ragged on a flat float64 / int32 array: block b is the
        n[b] x n[b] matrix at element offset[b] (any order, gaps and overlaps
        allowed).  tour_stride None: (largest n in 2..20) + 1.  out: optional
        (cost, tours, status) arrays to write into.  -> (cost, tours, status)."""
        dist = np.ascontiguousarray(dist)
        if dist.dtype != np.int32:
            dist = np.ascontiguousarray(dist, dtype=np.float64)
        dtype = I32 if dist.dtype == np.int32 else F64
        offset = np.ascontiguousarray(offset, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        B = len(n)
        assert len(offset) == B
        if tour_stride is None:
            ok = n[(n >= 2) & (n <= MAX_CITIES)]
            tour_stride = int(ok.max()) + 1 if ok.size else 1
        if out is None:
            cost = np.zeros(B, dtype=dist.dtype)
            tour = np.full((B, tour_stride), -1, dtype=np.int32)
            status = np.zeros(B, dtype=np.int32)
        else:
            cost, tour, status = out
            assert cost.dtype == dist.dtype and tour.dtype == np.int32 and status.dtype == np.int32
            assert cost.shape == (B,) and tour.shape == (B, tour_stride) and status.shape == (B,)
            assert cost.flags.c_contiguous and tour.flags.c_contiguous and status.flags.c_contiguous
        rc = lib().tspgpu_solve_ragged(self.handle, dist.ctypes.data, dtype, offset.ctypes.data_as(
            ctypes.POINTER(ctypes.c_int64)), _ip(n), B, cost.ctypes.data, _ip(tour), tour_stride, _ip(status))
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_ragged")
        return cost, tour, status

    def solve_ragged_device(self, d_dist_ptr: int, dtype: int, offset, n, d_cost_ptr: int, d_tour_ptr: int,
                            tour_stride: int, d_status_ptr: int, stream_ptr: int = 0):
        """tspgpu_solve_ragged_device: device pointers for dist / cost / tour
        (B x tour_stride) / status; offset and n are host arrays (read before
        this returns).  Asynchronous on stream_ptr."""
        offset = np.ascontiguousarray(offset, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        assert len(offset) == len(n)
        rc = lib().tspgpu_solve_ragged_device(self.handle, d_dist_ptr, dtype, offset.ctypes.data_as(
            ctypes.POINTER(ctypes.c_int64)), _ip(n), len(n), d_cost_ptr, d_tour_ptr, tour_stride, d_status_ptr,
            stream_ptr)
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_ragged_device")

    def last_grid(self) -> int:
        return lib().tspgpu_last_grid(self.handle)

    def last_variant(self) -> int:
        """K1 variant of the last batched launch (6: hk_sub_kernel; 4, 2: heldkarp_kernel; 0: n = 2)."""
        return lib().tspgpu_last_variant(self.handle)

    def k1_split_timing(self, enable: bool = True):
        """Record an event between variant 6's forward and backtracking kernels."""
        self._check(lib().tspgpu_k1_split_timing(self.handle, int(enable)), "tspgpu_k1_split_timing")

    def k1_last_split_ms(self):
        """(forward_ms, backtrack_ms) of the last variant-6 launch (waits for it)."""
        f, b = ctypes.c_float(), ctypes.c_float()
        self._check(lib().tspgpu_k1_last_split_ms(self.handle, ctypes.byref(f), ctypes.byref(b)),
                    "tspgpu_k1_last_split_ms")
        return f.value, b.value

    def _check(self, rc, what):
        if rc:
            raise TspGpuError(rc, what)

    def alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        self._check(lib().tspgpu_device_alloc(self.handle, nbytes, ctypes.byref(p)), "tspgpu_device_alloc")
        return p.value

    def free(self, ptr: int):
        self._check(lib().tspgpu_device_free(self.handle, ptr), "tspgpu_device_free")

    def upload(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self._check(lib().tspgpu_memcpy_htod(self.handle, p, arr.ctypes.data, arr.nbytes), "tspgpu_memcpy_htod")
        return p

    def download(self, ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self._check(lib().tspgpu_memcpy_dtoh(self.handle, out.ctypes.data, ptr, out.nbytes), "tspgpu_memcpy_dtoh")
        return out

    @property
    def stream(self) -> int:
        return lib().tspgpu_stream(self.handle) or 0

    def synchronize(self, stream: int | None = None):
        if stream is None:
            self._check(lib().tspgpu_synchronize(self.handle), "tspgpu_synchronize")
        else:
            self._check(lib().tspgpu_stream_synchronize(self.handle, stream), "tspgpu_stream_synchronize")

    def stream_create(self) -> int:
        s = ctypes.c_void_p()
        self._check(lib().tspgpu_stream_create(self.handle, ctypes.byref(s)), "tspgpu_stream_create")
        return s.value

    def stream_destroy(self, stream: int):
        self._check(lib().tspgpu_stream_destroy(self.handle, stream), "tspgpu_stream_destroy")

    def timer_start(self):
        self._check(lib().tspgpu_timer_start(self.handle), "tspgpu_timer_start")

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        self._check(lib().tspgpu_timer_stop(self.handle, ctypes.byref(ms)), "tspgpu_timer_stop")
        return ms.value

    def solve_instance(self, dist):
        """K1-wide: one instance over the whole GPU -> (cost, tour (n+1,), kernel ms)."""
        d = np.ascontiguousarray(dist, dtype=np.float64)
        n = d.shape[0]
        cost, ms = ctypes.c_double(), ctypes.c_double()
        tour = np.zeros(n + 1, dtype=np.int32)
        rc = lib().tspgpu_solve_instance(self.handle, _dp(d), n, ctypes.byref(cost), _ip(tour), ctypes.byref(ms))
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_instance")
        return cost.value, tour, ms.value

    def solve_instance_i32(self, dist):
        """K1-wide on int32 distances (the int32 table) -> (int cost, tour (n+1,) int32, kernel ms)."""
        d = np.ascontiguousarray(dist, dtype=np.int32)
        n = d.shape[0]
        cost, ms = ctypes.c_int32(), ctypes.c_double()
        tour = np.zeros(n + 1, dtype=np.int32)
        rc = lib().tspgpu_solve_instance_i32(self.handle, _ip(d), n, ctypes.byref(cost), _ip(tour), ctypes.byref(ms))
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_instance_i32")
        return int(cost.value), tour, ms.value

    def wide_last_dtype(self) -> int:
        """Value type of this context's last K1-wide launch (F64, I32; -1: none yet)."""
        return lib().tspgpu_wide_last_dtype(self.handle)

    def merge(self, p1, c1, p2, c2):
        """K3 mergeBlocks: paths are lists of (id, x, y) -> (merged path, cost)."""
        a1, _, _ = cities_array([p1])
        a2, _, _ = cities_array([p2])
        out = (City * (len(p1) + len(p2)))()
        cost = ctypes.c_double()
        rc = lib().tspgpu_merge(self.handle, a1, len(p1), c1, a2, len(p2), c2, out, ctypes.byref(cost))
        if rc < 0:
            raise TspGpuError(rc, "tspgpu_merge")
        return [(out[i].id, out[i].x, out[i].y) for i in range(rc)], cost.value

    def reduce(self, paths, costs, nprocs: int):
        """K3 reduction: paths (B lists of L cities), costs (B,) -> (final cost, log text)."""
        B, L = len(paths), len(paths[0])
        flat, _, _ = cities_array(paths)
        c = np.ascontiguousarray(costs, dtype=np.float64)
        final = ctypes.c_double()
        log = ctypes.create_string_buffer(1 << 20)
        rc = lib().tspgpu_reduce(self.handle, flat, L, _dp(c), B, nprocs, ctypes.byref(final), log, len(log))
        if rc:
            raise TspGpuError(rc, "tspgpu_reduce")
        return final.value, log.value.decode()

    @staticmethod
    def _tour_capacity(B: int, L: int, nprocs: int) -> int:
        """Room for rank 0's final path: every city and the closing one at one
        rank; the reference's stale receive lists repeat cities for more (the
        length grows by about 1.31 per tree round), so (2 + log2 P) times the
        cities, as bin/tsp sizes it."""
        return B * L * (2 + (nprocs.bit_length() - 1) if nprocs > 1 else 1) + 1

    def reduce_path(self, paths, costs, nprocs: int, path_cap: int | None = None):
        """K3 reduction with the merged tour (tspgpu_reduce_path): paths (B lists
        of L cities), costs (B,) -> (final cost, log text, rank 0's final path
        as a list of (id, x, y)).  path_cap None: room for (2 + log2 nprocs)
        times the cities, so one reduction gives the tour; only if that is
        ever short is the reduction run a second time with the reported
        length.  A given path_cap below the length raises -ENOSPC, with the
        full length in the error's path_len and the first path_cap cities in
        its path (path_cap 0 is the length query: it still runs the whole
        reduction)."""
        B, L = len(paths), len(paths[0])
        flat, _, _ = cities_array(paths)
        c = np.ascontiguousarray(costs, dtype=np.float64)

        def call(out, cap):
            final, plen = ctypes.c_double(), ctypes.c_int(-1)
            log = ctypes.create_string_buffer(1 << 20)
            rc = lib().tspgpu_reduce_path(self.handle, flat, L, _dp(c), B, nprocs, ctypes.byref(final), out, cap,
                                          ctypes.byref(plen), log, len(log))
            return rc, final.value, log.value.decode(), plen.value

        return self._path_result("tspgpu_reduce_path", call, path_cap, self._tour_capacity(B, L, nprocs))

    def _path_result(self, what, call, path_cap, generous):
        retry = path_cap is None
        if retry:
            path_cap = generous
        while True:
            out = (City * max(1, path_cap))()
            rc, final, log, plen = call(out if path_cap > 0 else None, path_cap)
            if rc == -errno.ENOSPC and retry and plen > path_cap:
                path_cap, retry = plen, False  # (the whole call again, once)
                continue
            path = [(out[i].id, out[i].x, out[i].y) for i in range(min(plen, path_cap) if plen >= 0 else 0)]
            if rc:
                err = TspGpuError(rc, what)
                err.path_len, err.path, err.cost, err.log = plen, path, final, log
                raise err
            return final, log, path

    def reduce_device(self, d_cities_ptr: int, d_tour_ptr: int, d_cost_ptr: int, d_status_ptr: int, n: int, B: int,
                      nprocs: int, d_path_ptr: int = 0, path_cap: int = 0, stream_ptr: int = 0):
        """tspgpu_reduce_device: K1's device outputs (cities B*n, tour rows of
        n+1, costs, statuses or 0) reduced without a visit to the host; the
        merged tour goes to d_path_ptr (device, path_cap cities; 0: not wanted).
        -> (final cost, log text, full path length).  A path_cap below the
        length raises -ENOSPC with cost, log and path_len on the error."""
        final, plen = ctypes.c_double(), ctypes.c_int(-1)
        log = ctypes.create_string_buffer(1 << 20)
        rc = lib().tspgpu_reduce_device(self.handle, d_cities_ptr, d_tour_ptr, d_cost_ptr, d_status_ptr or None, n, B,
                                        nprocs, ctypes.byref(final), d_path_ptr or None, path_cap,
                                        ctypes.byref(plen), log, len(log), stream_ptr or None)
        if rc:
            err = TspGpuError(rc, "tspgpu_reduce_device")
            err.path_len, err.cost, err.log = plen.value, final.value, log.value.decode()
            raise err
        return final.value, log.value.decode(), plen.value

    def reduce_device_last_ms(self) -> float:
        """Device time (HIP events) of the last reduce_device's gather, summary and uniqueness kernels."""
        ms = ctypes.c_double()
        self._check(lib().tspgpu_reduce_device_last_ms(self.handle, ctypes.byref(ms)), "tspgpu_reduce_device_last_ms")
        return ms.value

    # ---- fixed-end shortest paths and the window refinement of a tour ----

    def solve_paths(self, dist: np.ndarray):
        """tspgpu_solve_paths: dist (B, w, w) float64 or int32, city 0 the fixed
        start and city w-1 the fixed end of every block -> (cost (B,) of dist's
        type, order (B, w) int32: 0, t1..tm, w-1, status (B,) int32).  Status
        0: the minimal left fold and K1's tie-broken order on the folded
        matrix; else a negative errno, cost NaN / -1 and an order row of -1.
        Row w-1 and column 0 of a matrix are never read."""
        dist = np.ascontiguousarray(dist)
        if dist.dtype != np.int32:
            dist = np.ascontiguousarray(dist, dtype=np.float64)
        B, w, _ = dist.shape
        cost = np.zeros(B, dtype=dist.dtype)
        order = np.full((B, w), -1, dtype=np.int32)
        status = np.zeros(B, dtype=np.int32)
        self._check(lib().tspgpu_solve_paths(self.handle, dist.ctypes.data, I32 if dist.dtype == np.int32 else F64, w,
                                             B, cost.ctypes.data, _ip(order), _ip(status)), "tspgpu_solve_paths")
        return cost, order, status

    def solve_paths_device(self, d_dist_ptr: int, dtype: int, w: int, nblocks: int, d_cost_ptr: int, d_order_ptr: int,
                           d_status_ptr: int, stream_ptr: int = 0):
        """tspgpu_solve_paths_device: device pointers for dist (B*w*w of dtype),
        cost, order (B x w int32) and status.  Asynchronous on stream_ptr."""
        self._check(lib().tspgpu_solve_paths_device(self.handle, d_dist_ptr, dtype, w, nblocks, d_cost_ptr,
                                                    d_order_ptr, d_status_ptr, stream_ptr or None),
                    "tspgpu_solve_paths_device")

    def solve_paths_cities(self, blocks):
        """tspgpu_solve_paths_cities: blocks of w cities (lists of (id, x, y), or
        a (ctypes City array, w, B) triple), the first the fixed start and the
        last the fixed end -> (cost, order, status) as solve_paths, on the
        matrices of distance_matrix() built on the device."""
        arr, w, B = blocks if isinstance(blocks, tuple) else cities_array(blocks)
        cost = np.zeros(B, dtype=np.float64)
        order = np.full((B, w), -1, dtype=np.int32)
        status = np.zeros(B, dtype=np.int32)
        self._check(lib().tspgpu_solve_paths_cities(self.handle, arr, w, B, _dp(cost), _ip(order), _ip(status)),
                    "tspgpu_solve_paths_cities")
        return cost, order, status

    def solve_paths_cities_device(self, d_cities_ptr: int, w: int, nblocks: int, d_cost_ptr: int, d_order_ptr: int,
                                  d_status_ptr: int, stream_ptr: int = 0):
        """tspgpu_solve_paths_cities_device: B*w City structs on the device ->
        cost, order and status on the device.  Synchronises the stream as
        distance_matrix_device does; the solve is left running."""
        self._check(lib().tspgpu_solve_paths_cities_device(self.handle, d_cities_ptr, w, nblocks, d_cost_ptr,
                                                           d_order_ptr, d_status_ptr, stream_ptr or None),
                    "tspgpu_solve_paths_cities_device")

    def refine_path(self, path, interior: int = 15, max_passes: int = 8):
        """tspgpu_refine_path: a path (list of (id, x, y), closing city included
        or not) -> (refined path, stats dict).  The path is tiled with windows
        of `interior` cities between two fixed ones, every window is solved
        exactly and the strictly shorter orders are spliced back; odd passes
        shift the windows by half.  Both end cities stay."""
        arr, L, _ = cities_array([path])
        out = (City * max(1, L))()
        st = RefineStats()
        self._check(lib().tspgpu_refine_path(self.handle, arr, L, interior, max_passes, out, ctypes.byref(st)),
                    "tspgpu_refine_path")
        return [(out[i].id, out[i].x, out[i].y) for i in range(L)], st.as_dict()

    def refine_path_device(self, d_path_ptr: int, L: int, interior: int = 15, max_passes: int = 8,
                           stream_ptr: int = 0):
        """tspgpu_refine_path_device: L City structs on the device, refined in
        place; synchronous -> stats dict."""
        st = RefineStats()
        self._check(lib().tspgpu_refine_path_device(self.handle, d_path_ptr, L, interior, max_passes, ctypes.byref(st),
                                                    stream_ptr or None), "tspgpu_refine_path_device")
        return st.as_dict()

    def two_opt_path(self, path, ring: int = 2, max_passes: int = 1000):
        """tspgpu_two_opt_path: a path (list of (id, x, y), closing city included
        or not) -> (path, stats dict).  Passes of 2-opt moves between spatial
        neighbours (cells within `ring` of each other on a grid of about L / 2
        cells): every position's best move is found on the device, the host
        accepts a disjoint set greedily by gain, the device reverses.  Ends on
        a pass that finds nothing or after max_passes.  Both end cities stay."""
        arr, L, _ = cities_array([path])
        out = (City * max(1, L))()
        st = TwoOptStats()
        self._check(lib().tspgpu_two_opt_path(self.handle, arr, L, ring, max_passes, out, ctypes.byref(st)),
                    "tspgpu_two_opt_path")
        return [(out[i].id, out[i].x, out[i].y) for i in range(L)], st.as_dict()

    def two_opt_path_device(self, d_path_ptr: int, L: int, ring: int = 2, max_passes: int = 1000,
                            stream_ptr: int = 0):
        """tspgpu_two_opt_path_device: L City structs on the device, improved in
        place; synchronous -> stats dict."""
        st = TwoOptStats()
        self._check(lib().tspgpu_two_opt_path_device(self.handle, d_path_ptr, L, ring, max_passes, ctypes.byref(st),
                                                     stream_ptr or None), "tspgpu_two_opt_path_device")
        return st.as_dict()

    def or_opt_path(self, path, ring: int = 2, max_seg: int = 3, max_passes: int = 1000):
        """tspgpu_or_opt_path: a path (list of (id, x, y), closing city included
        or not) -> (path, stats dict).  Passes of Or-opt moves between spatial
        neighbours (the 2-opt stage's grid): segments of up to max_seg cities
        are taken out and put back, either way round, next to a city within
        `ring` cells; every position's best move is found on the device, the
        host accepts a disjoint set greedily by gain, the device rotates.
        Ends on a pass that finds nothing or after max_passes.  Both end
        cities stay."""
        arr, L, _ = cities_array([path])
        out = (City * max(1, L))()
        st = OrOptStats()
        self._check(lib().tspgpu_or_opt_path(self.handle, arr, L, ring, max_seg, max_passes, out, ctypes.byref(st)),
                    "tspgpu_or_opt_path")
        return [(out[i].id, out[i].x, out[i].y) for i in range(L)], st.as_dict()

    def or_opt_path_device(self, d_path_ptr: int, L: int, ring: int = 2, max_seg: int = 3, max_passes: int = 1000,
                           stream_ptr: int = 0):
        """tspgpu_or_opt_path_device: L City structs on the device, improved in
        place; synchronous -> stats dict."""
        st = OrOptStats()
        self._check(lib().tspgpu_or_opt_path_device(self.handle, d_path_ptr, L, ring, max_seg, max_passes,
                                                    ctypes.byref(st), stream_ptr or None), "tspgpu_or_opt_path_device")
        return st.as_dict()

    def _improved(self, result, two_opt: int, refine: int, or_opt: int = 0):
        """(final, log, tour) -> the same with the tour improved and the stats
        of the stages that ran behind it: 2-opt's, Or-opt's, the refinement's."""
        final, log, path = result
        stats = ()
        if two_opt:
            path, st = self.two_opt_path(path, 2, two_opt)
            stats += (st,)
        if or_opt:
            path, st = self.or_opt_path(path, 2, 3, or_opt)
            stats += (st,)
        if refine:
            path, st = self.refine_path(path, refine)
            stats += (st,)
        return (final, log, path) + stats

    def pipeline_cities(self, blocks, nprocs: int, path_cap: int | None = None, refine: int = 0, two_opt: int = 0,
                        or_opt: int = 0):
        """tspgpu_pipeline_cities: blocks (lists of (id, x, y), or a (ctypes City
        array, n, B) triple) -> (final cost, log text, merged tour as a list of
        (id, x, y)): block search and merges on the device, only the costs
        visit the host in between.  path_cap None: room for (2 + log2 nprocs)
        times the cities, so one run gives the tour; only if that is ever
        short does the whole pipeline run a second time with the reported
        length.  two_opt = passes > 0: two_opt_path(tour, 2, passes) on the
        merged tour; or_opt = passes > 0: or_opt_path(tour, 2, 3, passes)
        behind it; refine = m > 0: refine_path(tour, m) behind both -> (final
        cost, log text, improved tour, then the stats dict of every stage
        that ran, in that order); the cost and the log stay the reference's."""
        if refine or two_opt or or_opt:
            return self._improved(self.pipeline_cities(blocks, nprocs, path_cap), two_opt, refine, or_opt)
        arr, n, B = blocks if isinstance(blocks, tuple) else cities_array(blocks)

        def call(out, cap):
            final, plen = ctypes.c_double(), ctypes.c_int(-1)
            log = ctypes.create_string_buffer(1 << 20)
            rc = lib().tspgpu_pipeline_cities(self.handle, arr, n, B, nprocs, ctypes.byref(final), out, cap,
                                              ctypes.byref(plen), log, len(log))
            return rc, final.value, log.value.decode(), plen.value

        return self._path_result("tspgpu_pipeline_cities", call, path_cap,
                                 self._tour_capacity(B, tour_length(n), nprocs))

    # ---- ragged blocks end to end (packed cities, blocks of different sizes) ----

    @staticmethod
    def _ns(n):
        return np.ascontiguousarray(n, dtype=np.int32)

    def distance_matrix_ragged_device(self, d_cities_ptr: int, n, d_dist_ptr: int, stream_ptr: int = 0):
        """tspgpu_distance_matrix_ragged_device: packed cities (block b has n[b],
        a host array) -> the packed matrices (block b at sum n[a]^2) at
        d_dist_ptr, each with the bits of distance_matrix() on that block."""
        n = self._ns(n)
        rc = lib().tspgpu_distance_matrix_ragged_device(self.handle, d_cities_ptr, _ip(n), len(n), d_dist_ptr,
                                                        stream_ptr or None)
        if rc:
            raise TspGpuError(rc, "tspgpu_distance_matrix_ragged_device")

    def solve_cities_ragged_device(self, d_cities_ptr: int, n, d_cost_ptr: int, d_tour_ptr: int, tour_stride: int,
                                   d_status_ptr: int, stream_ptr: int = 0):
        """tspgpu_solve_cities_ragged_device: packed cities on the device -> cost
        (B float64), tours (B x tour_stride int32) and status (B int32) on the
        device, under the ragged contract."""
        n = self._ns(n)
        rc = lib().tspgpu_solve_cities_ragged_device(self.handle, d_cities_ptr, _ip(n), len(n), d_cost_ptr, d_tour_ptr,
                                                     tour_stride, d_status_ptr, stream_ptr or None)
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_cities_ragged_device")

    def solve_cities_ragged(self, blocks, tour_stride: int | None = None):
        """tspgpu_solve_cities_ragged: blocks of different sizes (lists of
        (id, x, y), or a (ctypes City array, n) pair from cities_array_ragged)
        -> (cost (B,), tours (B, tour_stride) padded with -1, status (B,)).
        tour_stride None: the largest n + 1."""
        arr, n = blocks if isinstance(blocks, tuple) else cities_array_ragged(blocks)
        n = self._ns(n)
        B = len(n)
        if tour_stride is None:
            tour_stride = int(n.max()) + 1 if B else 1
        cost = np.zeros(B, dtype=np.float64)
        tour = np.full((B, tour_stride), -1, dtype=np.int32)
        status = np.zeros(B, dtype=np.int32)
        rc = lib().tspgpu_solve_cities_ragged(self.handle, arr, _ip(n), B, _dp(cost), _ip(tour), tour_stride,
                                              _ip(status))
        if rc:
            raise TspGpuError(rc, "tspgpu_solve_cities_ragged")
        return cost, tour, status

    def reduce_ragged_device(self, d_cities_ptr: int, n, d_tour_ptr: int, tour_stride: int, d_cost_ptr: int,
                             d_status_ptr: int, nprocs: int, d_path_ptr: int = 0, path_cap: int = 0,
                             stream_ptr: int = 0):
        """tspgpu_reduce_ragged_device: the outputs of solve_cities_ragged_device
        reduced without a visit to the host -> (final cost, log text, full
        path length); the merged tour goes to d_path_ptr.  A path_cap below
        the length raises -ENOSPC with cost, log and path_len on the error."""
        n = self._ns(n)
        final, plen = ctypes.c_double(), ctypes.c_int(-1)
        log = ctypes.create_string_buffer(1 << 20)
        rc = lib().tspgpu_reduce_ragged_device(self.handle, d_cities_ptr, _ip(n), d_tour_ptr, tour_stride, d_cost_ptr,
                                               d_status_ptr or None, len(n), nprocs, ctypes.byref(final),
                                               d_path_ptr or None, path_cap, ctypes.byref(plen), log, len(log),
                                               stream_ptr or None)
        if rc:
            err = TspGpuError(rc, "tspgpu_reduce_ragged_device")
            err.path_len, err.cost, err.log = plen.value, final.value, log.value.decode()
            raise err
        return final.value, log.value.decode(), plen.value

    def reduce_ragged(self, paths, costs, nprocs: int, path_cap: int | None = None):
        """tspgpu_reduce_ragged: paths of different lengths (B lists of >= 2
        cities), costs (B,) -> (final cost, log text, rank 0's final path);
        path_cap as for reduce_path."""
        flat, lens = cities_array_ragged(paths)
        c = np.ascontiguousarray(costs, dtype=np.float64)
        B = len(lens)

        def call(out, cap):
            final, plen = ctypes.c_double(), ctypes.c_int(-1)
            log = ctypes.create_string_buffer(1 << 20)
            rc = lib().tspgpu_reduce_ragged(self.handle, flat, _ip(lens), _dp(c), B, nprocs, ctypes.byref(final), out,
                                            cap, ctypes.byref(plen), log, len(log))
            return rc, final.value, log.value.decode(), plen.value

        return self._path_result("tspgpu_reduce_ragged", call, path_cap,
                                 self._tour_capacity(1, int(lens.sum()), nprocs))

    def pipeline_cities_ragged(self, blocks, nprocs: int, path_cap: int | None = None, refine: int = 0,
                               two_opt: int = 0, or_opt: int = 0):
        """tspgpu_pipeline_cities_ragged: blocks of different sizes (lists of
        (id, x, y), or a (ctypes City array, n) pair) -> (final cost, log
        text, merged tour as a list of (id, x, y)); path_cap, refine, two_opt
        and or_opt as for pipeline_cities."""
        if refine or two_opt or or_opt:
            return self._improved(self.pipeline_cities_ragged(blocks, nprocs, path_cap), two_opt, refine, or_opt)
        arr, n = blocks if isinstance(blocks, tuple) else cities_array_ragged(blocks)
        n = self._ns(n)
        total = int(sum(tour_length(int(k)) for k in n))

        def call(out, cap):
            final, plen = ctypes.c_double(), ctypes.c_int(-1)
            log = ctypes.create_string_buffer(1 << 20)
            rc = lib().tspgpu_pipeline_cities_ragged(self.handle, arr, _ip(n), len(n), nprocs, ctypes.byref(final), out,
                                                     cap, ctypes.byref(plen), log, len(log))
            return rc, final.value, log.value.decode(), plen.value

        return self._path_result("tspgpu_pipeline_cities_ragged", call, path_cap,
                                 self._tour_capacity(1, total, nprocs))

    def device_info(self):
        cu = ctypes.c_int()
        name = ctypes.create_string_buffer(256)
        self._check(lib().tspgpu_device_info(self.handle, ctypes.byref(cu), name, 256), "tspgpu_device_info")
        return cu.value, name.value.decode()


def _search_dist(dist):
    """(n, n) matrix -> (contiguous array, dtype code): float -> F64, integer -> I32."""
    dist = np.asarray(dist)
    if np.issubdtype(dist.dtype, np.integer):
        return np.ascontiguousarray(dist, dtype=np.int32), I32
    return np.ascontiguousarray(dist, dtype=np.float64), F64


def cost_bits(cost, dtype: int) -> int:
    """The 64-bit incumbent word of a cost (f64 IEEE bits or the integer)."""
    if dtype == F64:
        return int(np.array([cost], dtype=np.float64).view(np.uint64)[0])
    return int(cost)


def bits_cost(bits: int, dtype: int):
    if dtype == F64:
        return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])
    return int(np.uint32(bits).view(np.int32))


def heuristic_tour(dist, first: int = 0, step: int = 1):
    """Multi-start tour (an upper bound): the start cities first, first+step, ...
    -> (cost, tour), or (None, None) when the range holds no start city."""
    d, dt = _search_dist(dist)
    n = d.shape[0]
    cost = ctypes.c_double()
    tour = np.zeros(n + 1, dtype=np.int32)
    rc = lib().tspgpu_heuristic_tour_starts(d.ctypes.data, dt, n, first, step, ctypes.byref(cost), _ip(tour))
    if rc == -errno.ENOENT:
        return None, None
    if rc:
        raise TspGpuError(rc, "tspgpu_heuristic_tour_starts")
    return cost.value, tour


def read_tsplib(path):
    """A TSPLIB file -> (name, int32 distance matrix): EDGE_WEIGHT_TYPE EUC_2D,
    CEIL_2D, ATT, GEO (TSPLIB95's integer distance functions; GEO degrees
    truncated like Concorde) or EXPLICIT (FULL_MATRIX, UPPER_ROW, LOWER_ROW,
    UPPER_DIAG_ROW, LOWER_DIAG_ROW).  The same reader as bin/tsp_search --tsplib
    (host/tsp_search.cpp); integer matrices run the exact integer mode."""
    import math

    hdr, coords, weights, section = {}, [], [], None
    for line in open(path):
        t = line.strip()
        if not t or t == "EOF":
            if t == "EOF":
                break
            continue
        if t.startswith("NODE_COORD_SECTION"):
            section = "coord"
            continue
        if t.startswith("EDGE_WEIGHT_SECTION"):
            section = "weight"
            continue
        if t.split()[0].endswith("_SECTION"):
            section = "skip"
            continue
        if section is None and ":" in t:
            k, v = t.split(":", 1)
            hdr[k.strip().upper()] = v.strip()
            continue
        if section == "coord":
            f = t.split()
            coords.append((float(f[1]), float(f[2])))
        elif section == "weight":
            weights.extend(int(float(x)) for x in t.split())
    n = int(hdr["DIMENSION"])
    kind = hdr.get("EDGE_WEIGHT_TYPE", "EUC_2D").upper()
    d = np.zeros((n, n), dtype=np.int64)
    if kind == "EXPLICIT":
        fmt = hdr.get("EDGE_WEIGHT_FORMAT", "FULL_MATRIX").upper()
        it = iter(weights)
        for i in range(n):
            if fmt == "FULL_MATRIX":
                cols = range(n)
            elif fmt == "UPPER_ROW":
                cols = range(i + 1, n)
            elif fmt == "LOWER_ROW":
                cols = range(i)
            elif fmt == "UPPER_DIAG_ROW":
                cols = range(i, n)
            elif fmt == "LOWER_DIAG_ROW":
                cols = range(i + 1)
            else:
                raise ValueError(f"EDGE_WEIGHT_FORMAT {fmt} not supported")
            for j in cols:
                d[i, j] = next(it)
                if fmt != "FULL_MATRIX":
                    d[j, i] = d[i, j]
    else:
        if len(coords) != n:
            raise ValueError("NODE_COORD_SECTION does not hold DIMENSION cities")

        def geo(v):
            deg = float(int(v))
            return 3.141592 * (deg + 5.0 * (v - deg) / 3.0) / 180.0

        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                (xi, yi), (xj, yj) = coords[i], coords[j]
                if kind == "GEO":
                    q1 = math.cos(geo(yi) - geo(yj))
                    q2 = math.cos(geo(xi) - geo(xj))
                    q3 = math.cos(geo(xi) + geo(xj))
                    d[i, j] = int(6378.388 * math.acos(0.5 * ((1.0 + q1) * q2 - (1.0 - q1) * q3)) + 1.0)
                elif kind == "ATT":
                    r = math.sqrt(((xi - xj) ** 2 + (yi - yj) ** 2) / 10.0)
                    t_ = int(r + 0.5)
                    d[i, j] = t_ + 1 if t_ < r else t_
                elif kind == "CEIL_2D":
                    d[i, j] = int(math.ceil(math.sqrt((xi - xj) ** 2 + (yi - yj) ** 2)))
                elif kind == "EUC_2D":
                    d[i, j] = int(math.sqrt((xi - xj) ** 2 + (yi - yj) ** 2) + 0.5)
                else:
                    raise ValueError(f"EDGE_WEIGHT_TYPE {kind} not supported")
    return hdr.get("NAME", os.path.basename(path)), d.astype(np.int32)


def _record_array(records):
    """A list of TourRecord, or a ctypes array of them as it is (Search.records(as_array=True): no
    per-record copy, millions of tied tours) -> the array to pass on."""
    if isinstance(records, ctypes.Array):
        return records
    return (TourRecord * max(1, len(records)))(*records)


def select_tour(dist, records, cost):
    """The DP's tie rule over the optimal set (tspgpu_select_tour)."""
    d, dt = _search_dist(dist)
    n = d.shape[0]
    arr = _record_array(records)
    tour = np.zeros(n + 1, dtype=np.int32)
    rc = lib().tspgpu_select_tour(d.ctypes.data, dt, n, arr, len(records), cost_bits(cost, dt), _ip(tour))
    if rc:
        raise TspGpuError(rc, "tspgpu_select_tour")
    return tour


def tie_key(tour):
    """The device tie rule's key (w0, w1) of a tour 0, t1..tN, 0 (tspgpu_tie_key)."""
    t = np.ascontiguousarray(tour, dtype=np.int32)
    w0, w1 = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().tspgpu_tie_key(len(t) - 1, _ip(t), ctypes.byref(w0), ctypes.byref(w1))
    if rc:
        raise TspGpuError(rc, "tspgpu_tie_key")
    return w0.value, w1.value


def tie_tour(dist, w0: int, w1: int, cost):
    """Decode + certify a tie key (tspgpu_tie_tour): (rc, tour); rc 0 = tsp()'s
    tour, -EAGAIN = a tour of that cost the DP may not pick."""
    d, dt = _search_dist(dist)
    n = d.shape[0]
    tour = np.zeros(n + 1, dtype=np.int32)
    rc = lib().tspgpu_tie_tour(d.ctypes.data, dt, n, w0, w1, cost_bits(cost, dt), _ip(tour))
    return rc, tour


def tie_tour_gpu(ctx: "Context", dist, w0: int, w1: int, cost):
    """tie_tour with the certificate's prefix DPs on the context's GPU
    (tspgpu_tie_tour_gpu): (rc, tour)."""
    d, dt = _search_dist(dist)
    n = d.shape[0]
    tour = np.zeros(n + 1, dtype=np.int32)
    rc = lib().tspgpu_tie_tour_gpu(ctx.handle, d.ctypes.data, dt, n, w0, w1, cost_bits(cost, dt), _ip(tour))
    return rc, tour


def tie_tour_records(ctx, dist, w0: int, w1: int, cost, records):
    """tie_tour with the certificate's prefix minima from the search's records
    (tspgpu_tie_tour_records): `records` must be every tour the search
    recorded at the optimum (Search.records(opt) without overflow, all
    shards).  ctx: the GPU DP for a prefix the records cannot decide (None:
    not certified).  -> (rc, tour)."""
    d, dt = _search_dist(dist)
    n = d.shape[0]
    tour = np.zeros(n + 1, dtype=np.int32)
    arr = _record_array(records)
    rc = lib().tspgpu_tie_tour_records(ctx.handle if ctx is not None else None, d.ctypes.data, dt, n, w0, w1,
                                       cost_bits(cost, dt), arr, len(records), _ip(tour))
    return rc, tour


class Search:
    """One instance (or shard `shard` of `nshards`) of the K2 search on a Context."""

    def __init__(self, ctx: "Context", dist, shard: int = 0, nshards: int = 1, depth: int = 0,
                 device_bound: bool = False, exhaustive: bool = False):
        """device_bound: the initial incumbent from the create launch's device
        heuristic (TSPGPU_SEARCH_DEVICE_BOUND) instead of set_bound.
        exhaustive: this shard of the exhaustive enumeration
        (TSPGPU_SEARCH_EXHAUSTIVE: no bound test; for 7 <= n <= 16 one launch
        over the prefixes p = i*nshards + shard, chain() runs it with zero
        hooks); set_bound(a real tour's cost, the same on every shard) first.
        Not together with device_bound (-EINVAL)."""
        self.dist, self.dtype = _search_dist(dist)
        self.n = self.dist.shape[0]
        h = ctypes.c_void_p()
        flags = (SEARCH_DEVICE_BOUND if device_bound else 0) | (SEARCH_EXHAUSTIVE if exhaustive else 0)
        rc = lib().tspgpu_search_create_ex(ctx.handle, self.dist.ctypes.data, self.dtype, self.n, shard, nshards,
                                           depth, flags, ctypes.byref(h))
        if rc:
            raise TspGpuError(rc, "tspgpu_search_create_ex")
        self.handle = h
        dep, items, local = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
        lib().tspgpu_search_info(h, ctypes.byref(dep), ctypes.byref(items), ctypes.byref(local))
        self.depth, self.items, self.local_items = dep.value, items.value, local.value

    def close(self):
        if self.handle:
            lib().tspgpu_search_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise TspGpuError(rc, what)

    def set_bound(self, bound: float):
        self._check(lib().tspgpu_search_set_bound(self.handle, float(bound)), "tspgpu_search_set_bound")

    def start(self):
        """Seed this shard's live prefixes."""
        self._check(lib().tspgpu_search_start(self.handle), "tspgpu_search_start")

    def step(self) -> int:
        """One round; returns the items pending for the next round."""
        p = ctypes.c_uint64()
        self._check(lib().tspgpu_search_step(self.handle, ctypes.byref(p)), "tspgpu_search_step")
        return p.value

    def run_all(self):
        self._check(lib().tspgpu_search_run_all(self.handle), "tspgpu_search_run_all")

    def chain(self, exchange_every: int = 0, hook=None, native_hook=None) -> bool:
        """This shard's whole search chained on the device with one
        synchronisation (tspgpu_search_chain); False: not a chain (too large:
        the shard is at its starting state; or too small to have a frontier
        level) — continue with start/step.  Every `exchange_every` levels an
        exchange of the device incumbent word is enqueued on the search's
        stream, by hook(stream, word) (Python) or native_hook = (address of a
        C tspgpu_level_hook, its user pointer), e.g. libtspcomm's in-stream
        RCCL all-reduce MIN; the same count on every shard either way."""
        done = ctypes.c_int()
        user = None
        if native_hook is not None:
            cb, user = LEVEL_HOOK(native_hook[0]), native_hook[1]
        elif hook is not None:
            cb = LEVEL_HOOK(lambda _u, st, w: hook(st, w))
        else:
            cb = LEVEL_HOOK()
        every = exchange_every if (hook is not None or native_hook is not None) else 0
        self._check(lib().tspgpu_search_chain(self.handle, every, cb, user, ctypes.byref(done)),
                    "tspgpu_search_chain")
        return bool(done.value)

    def tie_slot(self, bits: int):
        """The device tie rule's least key at cost word `bits` on this shard:
        (found, w0, w1, overflow)."""
        t = TieSlot()
        self._check(lib().tspgpu_search_tie_slot(self.handle, bits, ctypes.byref(t)), "tspgpu_search_tie_slot")
        return bool(t.found), int(t.w0), int(t.w1), bool(t.overflow)

    def timing(self):
        ms, rounds = ctypes.c_double(), ctypes.c_int()
        self._check(lib().tspgpu_search_timing(self.handle, ctypes.byref(ms), ctypes.byref(rounds)),
                    "tspgpu_search_timing")
        return ms.value, rounds.value

    @property
    def incumbent_ptr(self) -> int:
        return lib().tspgpu_search_incumbent_device(self.handle)

    def counters(self):
        inc, nodes, recs = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().tspgpu_search_counters(self.handle, ctypes.byref(inc), ctypes.byref(nodes),
                                                 ctypes.byref(recs)), "tspgpu_search_counters")
        return inc.value, nodes.value, recs.value

    def reset_records(self, capacity: int = 0):
        self._check(lib().tspgpu_search_reset_records(self.handle, capacity), "tspgpu_search_reset_records")

    def records(self, bits: int, as_array: bool = False):
        """Recorded tours whose cost word equals `bits`: a list of TourRecord,
        or (as_array) the ctypes array itself, which select_tour and
        tie_tour_records take without a copy per record."""
        cnt = ctypes.c_int()
        rc = lib().tspgpu_search_records(self.handle, bits, None, 0, ctypes.byref(cnt))
        if rc and rc != -errno.ENOSPC:
            raise TspGpuError(rc, "tspgpu_search_records")
        arr = (TourRecord * cnt.value)() if as_array else (TourRecord * max(1, cnt.value))()
        self._check(lib().tspgpu_search_records(self.handle, bits, arr if cnt.value else None, cnt.value,
                                                ctypes.byref(cnt)), "tspgpu_search_records")
        return arr if as_array else list(arr[:cnt.value])


def search_solve(ctx: "Context", dist, exhaustive: bool = False):
    """One instance on one GPU: (cost, tour (n+1,), stats dict).  exhaustive:
    enumerate every tour (no bound; tspgpu_search_enumerate)."""
    d, dt = _search_dist(dist)
    n = d.shape[0]
    cost = ctypes.c_double()
    tour = np.zeros(n + 1, dtype=np.int32)
    st = SearchStats()
    fn = lib().tspgpu_search_enumerate if exhaustive else lib().tspgpu_search_solve
    rc = fn(ctx.handle, d.ctypes.data, dt, n, ctypes.byref(cost), _ip(tour), ctypes.byref(st))
    if rc:
        raise TspGpuError(rc, "tspgpu_search_enumerate" if exhaustive else "tspgpu_search_solve")
    c = cost.value if dt == F64 else int(cost.value)
    return c, tour, st.as_dict()


def errno_name(code: int) -> str:
    return errno.errorcode.get(-code, str(code))
