"""bin/tsp_search --solver enum --gpus G: the exhaustive enumeration over G
shards of one process (the shards share the device when it has fewer GPUs:
host exchange), against K1 and against the one-GPU enumeration."""
import math
import os
import subprocess

import pytest

import tspgpu

BIN = os.path.join(os.path.dirname(tspgpu.TSP_BIN), "tsp_search")


def run(*args, timeout=120):
    p = subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def answer(out):
    return [ln for ln in out.splitlines() if ln.startswith(("optimal cost ", "tour "))]


@pytest.mark.gpu
def test_enum_over_three_shards():
    inst = ("--random", 12, "--seed", 3)
    rc, out, err = run(*inst, "--solver", "enum", "--gpus", 3, "--verify")
    assert rc == 0, err
    lines = out.splitlines()
    assert lines[0] == "cities 12  mode f64  solver enum  gpus 3", out
    assert "K1 check: identical cost and tour" in out
    assert any(ln.startswith("winner ") and ln.endswith("chained 1") for ln in lines), out
    tours = [ln for ln in lines if ln.startswith("tours ")]
    assert len(tours) == 1, out
    f = tours[0].split()
    assert int(f[1]) == math.factorial(11) and f[3] == "Gtours/s" and float(f[2]) > 0, tours
    assert f[4:8] == ["shard", "kernel", "ms", "min/max"], tours
    lo, hi = map(float, f[8].split("/"))
    assert 0 < lo <= hi
    # one GPU: the one-shot's output (no shard lines), the same answer
    rc1, out1, err1 = run(*inst, "--solver", "enum", "--gpus", 1)
    assert rc1 == 0, err1
    assert out1.splitlines()[0] == "cities 12  mode f64  solver enum  gpus 1", out1
    assert not any(ln.startswith(("tours ", "winner ")) for ln in out1.splitlines()), out1
    assert answer(out1) == answer(out) and len(answer(out)) == 2
