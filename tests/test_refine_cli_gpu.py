"""bin/tsp with TSP_REFINE=m: stdout stays the reference's (byte for byte, the
run's own milliseconds apart, which differ between any two runs), the tour file
holds the refined tour, and stderr gains the one line with the lengths."""
import os
import re
import subprocess

import pytest

import oracle_py as O
import tspgpu

pytestmark = pytest.mark.gpu
MS = re.compile(r"^TSP ran in \d+ ms ", re.M)
LINE = re.compile(r"^tsp refine: m 15 \| tour length ([0-9.]+) -> ([0-9.]+) \| (\d+) passes, (\d+) windows solved, "
                  r"(\d+) replaced, (\d+) skipped, gain ([0-9.]+)$", re.M)


def run_tsp(args, tour_file, extra):
    env = dict(os.environ, TSP_NPROCS="1", TSP_TOUR_OUT=str(tour_file), TSP_DEVICE_PIPELINE="1")
    for k in ("PMI_SIZE", "PMI_RANK", "OMPI_COMM_WORLD_SIZE", "OMPI_COMM_WORLD_RANK", "TSP_HOST_MERGE", "TSP_GPUS",
              "TSP_REFINE", "TSP_REFINE_PASSES", "TSP_STATS"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([tspgpu.TSP_BIN, *map(str, args)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    ids = [int(t) for t in open(tour_file).read().split()]
    return MS.sub("TSP ran in <ms> ms ", p.stdout), ids, p.stderr


def test_refined_tour_file_and_untouched_stdout(gpu_ctx, tmp_path):
    args = (8, 64, 1000, 1000)
    out0, ids0, err0 = run_tsp(args, tmp_path / "plain.txt", {})
    out1, ids1, err1 = run_tsp(args, tmp_path / "refined.txt", {"TSP_REFINE": "15"})
    assert out1 == out0 and "tsp refine" not in err0
    # the library's two steps on the same batch
    _, _, tour = gpu_ctx.pipeline_cities(O.generate(*args), 1)
    assert ids0 == [c[0] for c in tour]
    want, stats = gpu_ctx.refine_path(tour, 15, 8)
    assert ids1 == [c[0] for c in want] and ids1 != ids0
    m = LINE.search(err1)
    assert m, err1
    assert m.group(1) == f"{tspgpu.path_length(tour):f}" and m.group(2) == f"{tspgpu.path_length(want):f}"
    assert [int(m.group(i)) for i in (3, 4, 5, 6)] == [stats[k] for k in ("passes", "windows", "replaced", "skipped")]
    assert m.group(7) == f"{stats['gain']:f}"
