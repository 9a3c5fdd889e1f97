"""The Python model of the path problem and the window refinement
(tests/refine_model.py) against its own definition, on the CPU.

The reduction: for w <= 9 the oracle's Held-Karp on the folded matrix gives,
bit for bit, the minimum over all interior permutations of the path's left
fold, and an order that attains it.  The refinement: on every input the GPU
tests use, the model terminates within max_passes, keeps the multiset of
cities and both ends, never lengthens a window, and REPLACES AT LEAST ONE
WINDOW (so the GPU comparison is not a comparison of untouched paths).  The
exceptions are the inputs that exist to replace none: paths too short for a
window (L < m+2: zero stats) and the tie-only lattice."""
import math

import numpy as np
import pytest

import oracle_py as O
import refine_model as R


def _matrices(w, kind, count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        if kind == "uniform":
            xy = rng.uniform(0, 1000, size=(w, 2))
        elif kind == "lattice":
            xy = rng.integers(0, 5, size=(w, 2)).astype(float)
        else:  # coincident: three sites only
            xy = rng.uniform(0, 1000, size=(3, 2))[rng.integers(0, 3, size=w)]
        yield O.distance_matrix([(i, xy[i, 0], xy[i, 1]) for i in range(w)])


@pytest.mark.parametrize("w", [4, 5, 6, 8, 9])
@pytest.mark.parametrize("kind", ["uniform", "lattice", "coincident"])
def test_reduction_equals_brute_force(w, kind):
    for D in _matrices(w, kind, 4 if w == 9 else 8, 17 * w):
        cost, order, st = R.solve_path(D)
        assert st == 0 and order[0] == 0 and order[-1] == w - 1
        assert sorted(order) == list(range(w))
        assert float(R.left_fold(D, order)) == cost  # the order attains the cost
        assert cost == R.brute_force(D)              # and no permutation is below it


def test_reduction_on_asymmetric_matrices_never_reads_row_end_or_column_start():
    rng = np.random.default_rng(5)
    for w in (4, 6, 8):
        D = rng.uniform(1, 100, size=(w, w))
        want = R.brute_force(D)
        D[w - 1, :] = math.nan
        D[:, 0] = -7.0
        cost, order, st = R.solve_path(D)
        assert st == 0 and cost == want


def test_pass_windows():
    assert R.pass_windows(2, 2, 0) == (0, 0) and R.pass_windows(4, 2, 0) == (0, 1)
    assert R.pass_windows(4, 2, 1) == (1, 0) and R.pass_windows(5, 2, 1) == (1, 1)
    assert R.pass_windows(600, 15, 0) == (0, 37) and R.pass_windows(600, 15, 1) == (8, 36)


def _check(name, must_replace):
    path, m, passes, out, stats = R.refined(name)
    L = len(path)
    assert 1 <= stats["passes"] <= passes or (stats["passes"] == 0 and R.pass_windows(L, m, 0)[1] == 0)
    assert sorted(out) == sorted(path) and out[0] == path[0] and out[-1] == path[-1]
    trace = []
    again, stats2 = R.refine(path, m, passes, trace)
    assert again == out and stats2 == stats  # deterministic
    for _, _, old, new, st, take in trace:
        assert take == (st == 0 and new < old)
    assert stats["gain"] >= 0.0
    if must_replace:
        assert stats["replaced"] >= 1 and stats["gain"] > 0.0
        assert R.path_length(out) < R.path_length(path)
    else:
        assert stats["replaced"] == 0 and out == path
    return stats


@pytest.mark.parametrize("name", sorted(R.REFINE_INPUTS))
def test_model_on_the_gpu_inputs(name):
    stats = _check(name, True)
    if name.startswith("outlier"):
        assert stats["skipped"] >= 1


@pytest.mark.parametrize("name", sorted(R.SMALL_INPUTS))
def test_model_on_the_small_inputs(name):
    path, m, _ = R.built(name)
    has_window = len(path) >= m + 2
    stats = _check(name, has_window)
    if not has_window:
        assert stats == {"passes": 0, "windows": 0, "replaced": 0, "skipped": 0, "gain": 0.0}


def test_tie_only_lattice_replaces_nothing():
    stats = _check(R.TIE_INPUT[0], False)
    assert stats["windows"] > 0 and stats["skipped"] == 0


def test_wide_input_replaces():
    path, m, passes = R.wide_input(13)  # (the builder's shape at a small CU count)
    out, stats = R.refine(path, m, passes)
    assert len(path) == 13 * 16 + 1 and stats["replaced"] >= 1 and sorted(out) == sorted(path)
