"""bin/tsp with TSP_DEVICE_PIPELINE=1 (block search and merges in one call,
K1's results kept on the GPU) against its default path: the same stdout apart
from the milliseconds, and the same merged tour in TSP_TOUR_OUT."""
import os
import re
import subprocess

import pytest

import tspgpu

pytestmark = pytest.mark.gpu
MS = re.compile(r"^TSP ran in \d+ ms ", re.M)


def run_tsp(args, tour_file, pipeline, P=1, extra=None):
    env = dict(os.environ, TSP_NPROCS=str(P), TSP_TOUR_OUT=str(tour_file), TSP_STATS="1")
    for k in ("PMI_SIZE", "PMI_RANK", "OMPI_COMM_WORLD_SIZE", "OMPI_COMM_WORLD_RANK", "TSP_DEVICE_PIPELINE",
              "TSP_HOST_MERGE", "TSP_GPUS"):
        env.pop(k, None)
    if pipeline:
        env["TSP_DEVICE_PIPELINE"] = "1"
    env.update(extra or {})
    p = subprocess.run([tspgpu.TSP_BIN, *map(str, args)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    ids = [int(t) for t in open(tour_file).read().split()]
    return MS.sub("TSP ran in <ms> ms ", p.stdout), ids, p.stderr


@pytest.mark.parametrize("args", [(8, 64, 1000, 1000), (16, 8, 1000, 1000)], ids=lambda a: "-".join(map(str, a)))
def test_pipeline_mode_prints_what_the_default_prints(tmp_path, args):
    n, B = args[:2]
    out0, ids0, err0 = run_tsp(args, tmp_path / "default.txt", False)
    out1, ids1, err1 = run_tsp(args, tmp_path / "pipeline.txt", True)
    assert out1 == out0 and "trip cost" in out0
    assert ids1 == ids0
    # P = 1: a closed tour that visits every id exactly once, plus the closing id
    for ids in (ids0, ids1):
        assert len(ids) == n * B + 1 and ids[0] == ids[-1] and sorted(ids[:-1]) == list(range(n * B))
    assert "device pipeline" in err1 and "device pipeline" not in err0 and "ignored" not in err0 + err1


def test_pipeline_mode_with_ranks_and_where_it_is_ignored(tmp_path):
    args = (8, 64, 1000, 1000)
    out0, ids0, _ = run_tsp(args, tmp_path / "default.txt", False, P=3)
    out1, ids1, err1 = run_tsp(args, tmp_path / "pipeline.txt", True, P=3)
    assert out1 == out0 and ids1 == ids0 and out0.count("process 0 is about to receive") == 1
    assert "device pipeline" in err1
    # two GPUs asked for: the switch is ignored, and the statistics line says so
    out2, ids2, err2 = run_tsp(args, tmp_path / "ignored.txt", True, P=3, extra={"TSP_GPUS": "2"})
    assert out2 == out0 and ids2 == ids0 and "TSP_DEVICE_PIPELINE ignored" in err2
