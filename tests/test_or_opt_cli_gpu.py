"""bin/tsp with TSP_OR_OPT=passes behind TSP_TWO_OPT: stdout stays the
reference's (byte for byte, the run's own milliseconds apart, which differ
between any two runs), the tour file holds what the library's calls give in
the same order, and stderr gains the one line with the lengths."""
import os
import re
import subprocess

import pytest

import oracle_py as O
import tspgpu

pytestmark = pytest.mark.gpu
MS = re.compile(r"^TSP ran in \d+ ms ", re.M)
LINE = re.compile(r"^tsp or-opt: ring (\d+), segments to (\d+) \| tour length ([0-9.]+) -> ([0-9.]+) \| (\d+) passes, "
                  r"(\d+) moves, gain ([0-9.]+)$", re.M)


def run_tsp(args, tour_file, extra):
    env = dict(os.environ, TSP_NPROCS="1", TSP_TOUR_OUT=str(tour_file), TSP_DEVICE_PIPELINE="1")
    for k in ("PMI_SIZE", "PMI_RANK", "OMPI_COMM_WORLD_SIZE", "OMPI_COMM_WORLD_RANK", "TSP_HOST_MERGE", "TSP_GPUS",
              "TSP_REFINE", "TSP_REFINE_PASSES", "TSP_TWO_OPT", "TSP_TWO_OPT_RING", "TSP_OR_OPT", "TSP_OR_OPT_RING",
              "TSP_OR_OPT_SEG", "TSP_STATS"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([tspgpu.TSP_BIN, *map(str, args)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    ids = [int(t) for t in open(tour_file).read().split()]
    return MS.sub("TSP ran in <ms> ms ", p.stdout), ids, p.stderr


def test_or_opt_tour_file_and_untouched_stdout(gpu_ctx, tmp_path):
    args = (8, 64, 1000, 1000)
    out0, ids0, err0 = run_tsp(args, tmp_path / "plain.txt", {})
    out1, ids1, err1 = run_tsp(args, tmp_path / "or_opt.txt", {"TSP_TWO_OPT": "1000", "TSP_OR_OPT": "1000"})
    assert out1 == out0 and "tsp or-opt" not in err0
    # the library's steps on the same batch
    _, _, tour = gpu_ctx.pipeline_cities(O.generate(*args), 1)
    assert ids0 == [c[0] for c in tour]
    tpath, _ = gpu_ctx.two_opt_path(tour, 2, 1000)
    want, stats = gpu_ctx.or_opt_path(tpath, 2, 3, 1000)
    assert ids1 == [c[0] for c in want] and ids1 != [c[0] for c in tpath]
    assert sorted(ids1) == sorted(ids0) and (ids1[0], ids1[-1]) == (ids0[0], ids0[-1])
    assert tspgpu.path_length(want) < tspgpu.path_length(tpath)
    m = LINE.search(err1)
    assert m, err1
    assert (m.group(1), m.group(2)) == ("2", "3")
    assert m.group(3) == f"{tspgpu.path_length(tpath):f}" and m.group(4) == f"{tspgpu.path_length(want):f}"
    assert [int(m.group(5)), int(m.group(6))] == [stats["passes"], stats["moves"]]
    assert m.group(7) == f"{stats['gain']:f}"
    assert err1.index("tsp two-opt: ring 2 ") < err1.index("tsp or-opt: ring 2, ")
    # between TSP_TWO_OPT and TSP_REFINE when all are set; ring and segment length are the caller's
    out2, ids2, err2 = run_tsp(args, tmp_path / "all.txt", {"TSP_TWO_OPT": "1000", "TSP_OR_OPT": "1000", "TSP_REFINE": "7",
                                                            "TSP_OR_OPT_RING": "1", "TSP_OR_OPT_SEG": "2"})
    want2, _ = gpu_ctx.or_opt_path(tpath, 1, 2, 1000)
    both, _ = gpu_ctx.refine_path(want2, 7)
    assert out2 == out0 and ids2 == [c[0] for c in both]
    assert err2.index("tsp two-opt: ring 2 ") < err2.index("tsp or-opt: ring 1, segments to 2 ") < err2.index(
        "tsp refine: m 7 ")
    # alone it runs on the merged tour
    out3, ids3, err3 = run_tsp(args, tmp_path / "alone.txt", {"TSP_OR_OPT": "3"})
    cut, _ = gpu_ctx.or_opt_path(tour, 2, 3, 3)
    assert out3 == out0 and ids3 == [c[0] for c in cut] and "tsp two-opt" not in err3
