"""The Python model of the 2-opt stage (tests/two_opt_model.py) against its own
contract, on the CPU.

two_opt() evaluates a pass as numpy arrays; plain_*() is the contract word
for word, quadratic, with no neighbour list.  Here the two are held against
each other, and on every input the GPU tests use the model keeps the cities
and both ends, folds its gain from the left, stops only where no candidate
with gain > 0 is left, does not depend on the order of the neighbour lists,
and APPLIES AT LEAST ONE MOVE and gets strictly shorter under
tspgpu.path_length (so the GPU comparison is not one of untouched paths).
The exceptions are the inputs that exist to move nothing."""
import errno
import math

import numpy as np
import pytest

import tspgpu
import two_opt_model as T

ZERO = {"passes": 0, "candidates": 0, "moves": 0, "gain": 0.0}


def test_grid_size():
    for L in list(range(1, 3000)) + [262145, 2 * 2048 * 2048 - 1, 2 * 2048 * 2048, 2**30]:
        g = T.grid_size(L)
        assert 1 <= g <= 2048
        assert g == 1 or 2 * g * g <= L
        assert g == 2048 or 2 * (g + 1) * (g + 1) > L
    assert T.grid_size(262145) == 362 and T.grid_size(2**30) == 2048


@pytest.mark.parametrize("name", sorted(T.IDLE_INPUTS))
def test_nothing_to_do(name):
    path, ring, passes, out, stats = T.solved(name)
    assert out == path
    assert stats == (ZERO if len(path) < 4 else dict(ZERO, passes=1))


@pytest.mark.parametrize("name", sorted(T.MOVING_INPUTS) + sorted(T.CUT_INPUTS))
def test_model_on_the_gpu_inputs(name):
    path, ring, passes, out, stats = T.solved(name)
    assert sorted(out) == sorted(path) and out[0] == path[0] and out[-1] == path[-1]
    trace = []
    again, stats2 = T.two_opt(path, ring, passes, trace=trace)
    assert again == out and stats2 == stats  # deterministic
    # the stats are the trace's: a left fold of the accepted gains in acceptance order
    fold = 0.0
    for accepted in trace:
        gains = [g for g, _, _ in accepted]
        assert gains == sorted(gains, reverse=True) and all(g > 0.0 for g in gains)
        spans = sorted((i, j) for _, i, j in accepted)
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))  # disjoint edge ranges
        for g in gains:
            fold = fold + g
    assert stats["gain"] == fold and stats["passes"] == len(trace)
    assert stats["moves"] == sum(len(a) for a in trace) >= 1
    assert tspgpu.path_length(out) < tspgpu.path_length(path)
    if name in T.CUT_INPUTS:
        assert stats["passes"] == passes and trace[-1]  # cut while moves were still found
    else:
        assert stats["passes"] < passes and not trace[-1]
        # the stop rule: re-enumerated by the definition, no candidate with gain > 0 is left
        assert T.plain_best_moves(path, _order_of(path, out), ring) == []


def _order_of(path, out):
    """The input index of the city at every output position (duplicates by
    first unused match: they share id and place, so either names the city)."""
    free = {}
    for k, c in enumerate(path):
        free.setdefault(c, []).append(k)
    return [free[c].pop(0) for c in out]


@pytest.mark.parametrize("name", ["L4", "L5", "bow-tie", "one-point-50", "lattice-scrambled-200", "closed-tour-251",
                                  "clustered-300", "scrambled-400-cut3"])
def test_vector_model_equals_the_plain_statement(name):
    path, ring, passes, out, stats = T.solved(name)
    pout, pstats = T.plain_two_opt(path, ring, passes)
    assert pout == out and pstats == stats


@pytest.mark.parametrize("name", ["scrambled-700", "reversed-sweep-2000", "scrambled-400-ring1", "scrambled-400-ring4",
                                  "generator-8x64"])
def test_first_pass_candidates_equal_the_plain_statement(name):
    """The larger inputs: the best move of every position under the input order."""
    path, ring, _ = T.built(name)
    path = list(path)
    _, cx, cy = T.cells(path)
    assert [cx.tolist(), cy.tolist()] == T.plain_cells(path)
    u, v = T.neighbour_pairs(cx, cy, ring)
    x = np.array([c[1] for c in path])
    y = np.array([c[2] for c in path])
    gain, i, j = T.best_moves(np.arange(len(path)), x, y, u, v)
    got = sorted(zip(gain.tolist(), i.tolist(), j.tolist()), key=lambda m: m[1])
    assert got == T.plain_best_moves(path, list(range(len(path))), ring) and got


@pytest.mark.parametrize("name", ["lattice-scrambled-200", "clustered-300", "scrambled-400", "closed-tour-251"])
def test_cell_list_order_does_not_matter(name):
    path, ring, passes, out, stats = T.solved(name)
    for seed in (1, 2):
        again, stats2 = T.two_opt(path, ring, passes, rng=np.random.default_rng(seed))
        assert again == out and stats2 == stats


def test_bow_tie_takes_its_one_move():
    path, ring, passes, out, stats = T.solved("bow-tie")
    trace = []
    T.two_opt(path, ring, passes, trace=trace)
    assert [[(i, j) for _, i, j in a] for a in trace] == [[T.BOW_TIE_MOVE], []]
    assert trace[0][0][0] == (math.sqrt(2.0) + math.sqrt(2.0)) - (1.0 + 1.0)
    assert out == [path[k] for k in (0, 1, 3, 2, 4, 5)]
    assert stats == {"passes": 2, "candidates": 1, "moves": 1, "gain": trace[0][0][0]}
    assert tspgpu.path_length(out) == 5.0


def test_first_legal_moves():
    for name, L in (("L4", 4), ("L5", 5)):
        path, ring, passes, out, stats = T.solved(name)
        assert [c[1] for c in out] == [float(k) for k in range(L)] and stats["moves"] == 1 and stats["passes"] == 2


def test_clustered_input_fills_one_cell():
    path = list(T.built("clustered-300")[0])
    g, cx, cy = T.cells(path)
    assert g == 12 and int(((cx == 0) & (cy == 0)).sum()) >= 200


def test_reversed_sweep_is_one_long_move():
    path, ring, passes, out, stats = T.solved("reversed-sweep-2000")
    trace = []
    T.two_opt(path, ring, passes, trace=trace)
    assert (199, 1700) in [(i, j) for _, i, j in trace[0]] and stats["passes"] <= 4
    assert [c[0] for c in out] == list(range(2000))


def test_refused_paths():
    ok = [(k, float(k), 1.0) for k in range(6)]
    for bad in (math.nan, math.inf, -math.inf):
        for at in (0, 3, 5):
            for axis in (1, 2):
                path = [list(c) for c in ok]
                path[at][axis] = bad
                assert T.two_opt([tuple(c) for c in path]) == (None, -errno.EINVAL)
    wide = [(0, -1.0e308, 0.0), (1, 1.0e308, 0.0), (2, 0.0, 0.0), (3, 1.0, 1.0)]
    assert T.two_opt(wide) == (None, -errno.ERANGE)
    square = [(0, -1.0e200, 0.0), (1, 1.0e200, 0.0), (2, 0.0, 0.0), (3, 1.0, 1.0)]  # ex finite, ex*ex not
    assert T.two_opt(square) == (None, -errno.ERANGE)
    assert T.two_opt([(0, math.nan, 0.0)]) == (None, -errno.EINVAL)  # (validated before "nothing to do")
