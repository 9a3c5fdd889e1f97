"""The Python model of the Or-opt stage (tests/or_opt_model.py) against its own
contract, on the CPU.

or_opt() evaluates a pass as numpy arrays; plain_or_opt() is the contract word
for word, with N tested by its definition.  Here the two are held against
each other, and on every input the GPU tests use the model keeps the cities
and both ends, folds its gain from the left, accepts disjoint ranges, stops
only where no candidate with gain > 0 is left, does not depend on the order of
the neighbour lists, and APPLIES AT LEAST ONE MOVE and gets strictly shorter
under tspgpu.path_length (so the GPU comparison is not one of untouched
paths).  The exceptions are the inputs that exist to move nothing.

The inputs are shown to be able to fail: each named wrong implementation of
the model (or_opt()'s `mutant`) gives another path on an input pinned here."""
import math

import numpy as np
import pytest

import or_opt_model as M
import tspgpu
import two_opt_model as T

ZERO = {"passes": 0, "candidates": 0, "moves": 0, "gain": 0.0}


@pytest.mark.parametrize("name", sorted(M.IDLE_INPUTS))
def test_nothing_to_do(name):
    path, ring, seg, passes, out, stats = M.solved(name)
    assert out == path
    assert stats == (ZERO if len(path) < 4 else dict(ZERO, passes=1))


def _order_of(path, out):
    """The input index of the city at every output position (duplicates by
    first unused match: they share id and place, so either names the city)."""
    free = {}
    for k, c in enumerate(path):
        free.setdefault(c, []).append(k)
    return [free[c].pop(0) for c in out]


@pytest.mark.parametrize("name", sorted(M.MOVING_INPUTS) + sorted(M.CUT_INPUTS))
def test_model_on_the_gpu_inputs(name):
    path, ring, seg, passes, out, stats = M.solved(name)
    assert sorted(out) == sorted(path) and out[0] == path[0] and out[-1] == path[-1]
    trace = []
    again, stats2 = M.or_opt(path, ring, seg, passes, trace=trace)
    assert again == out and stats2 == stats  # deterministic
    # the stats are the trace's: a left fold of the accepted gains in acceptance order
    fold = 0.0
    for accepted in trace:
        gains = [m[0] for m in accepted]
        assert gains == sorted(gains, reverse=True) and all(g > 0.0 for g in gains)
        spans = sorted(M.move_range(a, k, t) for _, _, a, k, t, _ in accepted)
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))  # disjoint edge ranges
        for _, s, a, k, t, rev in accepted:
            assert 1 <= k <= seg and 1 <= a and a + k - 1 <= len(path) - 2 and 0 <= t <= len(path) - 2
            assert not a - 1 <= t <= a + k - 1 and s in (a, a + k - 1) and (k > 1 or rev == 0)
        for g in gains:
            fold = fold + g
    assert stats["gain"] == fold and stats["passes"] == len(trace)
    assert stats["moves"] == sum(len(a) for a in trace) >= 1
    assert tspgpu.path_length(out) < tspgpu.path_length(path)
    if name in M.CUT_INPUTS:
        assert stats["passes"] == passes and trace[-1]  # cut while moves were still found
    else:
        assert stats["passes"] < passes and not trace[-1]
        if len(path) <= 700:  # the stop rule: re-enumerated by the definition, no candidate with gain > 0 is left
            assert M.plain_best_moves(path, _order_of(path, out), ring, seg) == []


@pytest.mark.parametrize("name", ["L4", "L5", "L6", "one-point-50", "2opt:closed-tour-251", "scrambled-400-cut3"])
def test_vector_model_equals_the_plain_statement(name):
    path, ring, seg, passes, out, stats = M.solved(name)
    pout, pstats = M.plain_or_opt(path, ring, seg, passes)
    assert pout == out and pstats == stats


@pytest.mark.parametrize("name", ["lattice-scrambled-200", "clustered-300", "2opt:scrambled-700", "scrambled-400-ring1",
                                  "scrambled-400-ring4", "scrambled-400-seg1", "scrambled-400-seg2",
                                  "2opt:generator-8x64"])
def test_first_pass_candidates_equal_the_plain_statement(name):
    """The longer runs: the best move of every position under the input order."""
    path, ring, seg, _ = M.built(name)
    path = list(path)
    g, cx, cy = T.cells(path)
    u, v = T.grid_neighbour_pairs(cx, cy, g, ring)
    x = np.array([c[1] for c in path])
    y = np.array([c[2] for c in path])
    got = sorted(zip(*(col.tolist() for col in M.best_moves(np.arange(len(path)), x, y, u, v, seg))),
                 key=lambda m: m[1])
    assert got == M.plain_best_moves(path, list(range(len(path))), ring, seg) and got


@pytest.mark.parametrize("name", ["lattice-scrambled-200", "2opt:clustered-300", "scrambled-400-cut3",
                                  "2opt:closed-tour-251"])
def test_pair_list_order_does_not_matter(name):
    path, ring, seg, passes, out, stats = M.solved(name)
    for seed in (1, 2):
        again, stats2 = M.or_opt(path, ring, seg, passes, rng=np.random.default_rng(seed))
        assert again == out and stats2 == stats


@pytest.mark.parametrize("name", sorted(M.OPTIMAL_INPUTS))
def test_or_opt_improves_what_two_opt_has_finished_with(name):
    path, ring, seg, passes, out, stats = M.solved(name)
    # nothing left for 2-opt under its own model
    assert T.two_opt(path, 2, 1)[1] == dict(ZERO, passes=1)
    assert stats["moves"] > 0 and stats["passes"] < passes
    # the left fold of the reference's distance in path order
    assert tspgpu.path_length(out) < tspgpu.path_length(path)


def test_the_smallest_paths_take_the_moves_they_are_named_for():
    """L = 4, 5, 6: one pass with one move each, k = 1, 2, 3, touching both
    fixed ends.  Inside so few positions the named move has a twin with the
    same result and the same gain (k cities past j others is j past k), so
    the named move is a candidate of the first pass, and what the model
    accepts gives the same path."""
    for name, L in (("L4", 4), ("L5", 5), ("L6", 6)):
        path, ring, seg, passes, out, stats = M.solved(name)
        assert len(path) == L and T.grid_size(L) == 1
        assert [c[1] for c in out] == [3.0 * t for t in range(L)] and stats["moves"] == 1 and stats["passes"] == 2
        cand = M.plain_best_moves(path, list(range(L)), ring, seg)
        a, k, t, rev = M.NAMED_MOVES[name]
        assert k == L - 3 and (a - 1 == 0 or t == 0) and (a + k - 1 == L - 2 or t == L - 2)
        assert (a, k, t, rev) in [m[2:] for m in cand]
        assert len({m[0] for m in cand}) == 1 and cand[0][0] == stats["gain"] == 10.0 * (L - 3)
        order = list(range(L))
        M.apply_move(order, a, k, t, rev)
        assert [path[c] for c in order] == out
    trace = []
    M.or_opt(*M.solved("L6")[:4], trace=trace)
    assert trace[0][0][2:] == (1, 3, 4, 1)  # the twin: reversed, into edge L - 2


def test_strays_are_one_long_rotation_each_way():
    want = [c[0] for c in M.curve()]
    for name, forward, k in (("stray-forward-2000", True, 1), ("stray-backward-2000", False, 1),
                             ("stray-three-reversed-2000", True, 3)):
        path, ring, seg, passes, out, stats = M.solved(name)
        trace = []
        M.or_opt(path, ring, seg, passes, trace=trace)
        assert [c[0] for c in out] == want and stats["moves"] == 1 and len(trace) == 2
        _, _, a, kk, t, rev = trace[0][0]
        lo, hi = M.move_range(a, kk, t)
        assert kk == k and rev == (k == 3) and (t > a) == forward and hi - lo > 1500  # past any workgroup


def test_the_tie_input_ties():
    """lattice-scrambled-200 is where "the smallest tuple on equal gains" and
    "s ascending on equal gains" decide."""
    path, ring, seg, _ = M.built("lattice-scrambled-200")
    path = list(path)
    g, cx, cy = T.cells(path)
    u, v = T.grid_neighbour_pairs(cx, cy, g, ring)
    x = np.array([c[1] for c in path])
    y = np.array([c[2] for c in path])
    order = np.arange(len(path))
    best = {}
    for gain, s, *move in set(zip(*(a.tolist() for a in M.improving_moves(order, x, y, u, v, seg)))):
        top = best.setdefault(s, [gain, set()])
        if gain > top[0]:
            top[0], top[1] = gain, {tuple(move)}
        elif gain == top[0]:
            top[1].add(tuple(move))
    assert sum(len(moves) >= 2 for _, moves in best.values()) >= 10
    gains = M.best_moves(order, x, y, u, v, seg)[0]
    assert len(gains) - len(set(gains.tolist())) >= 20  # candidates whose gain another position has too


def test_one_move_is_reported_by_both_of_its_ends():
    path, ring, seg, _ = M.built("scrambled-400")
    path = list(path)
    cand = M.plain_best_moves(path, list(range(len(path))), ring, seg)
    moves = [m[2:] for m in cand]
    assert len(moves) - len(set(moves)) >= 10


@pytest.mark.parametrize("mutant, name", [("no-trailing", "scrambled-400-cut3"), ("no-trailing", "lattice-scrambled-200"),
                                          ("no-reversed", "2opt:closed-tour-251"),
                                          ("ties-largest", "lattice-scrambled-200"),
                                          ("wide-exclusion", "L4"), ("wide-exclusion", "L6")])
def test_inputs_notice_a_wrong_implementation(mutant, name):
    """no-trailing: the segments that end on s are not tried; no-reversed: no
    reversed insertion; ties-largest: the largest tuple on equal gains;
    wide-exclusion: t = a-2 and t = h+1 are taken for illegal."""
    path, ring, seg, passes, out, stats = M.solved(name)
    mout, mstats = M.or_opt(path, ring, seg, passes, mutant=mutant)
    assert sorted(mout) == sorted(path)  # a valid path all the same: only the comparison can tell
    assert mout != out


@pytest.mark.parametrize("exponent", [500, -500])
def test_scaled_inputs_are_the_base_input_times_a_power_of_two(exponent):
    _, _, _, _, bout, bstats = M.solved(M.SCALED_BASE)
    path, ring, seg, passes, out, stats = M.solved(f"{M.SCALED_BASE}-x2^{exponent}")
    assert T.validate(path) == 0
    assert [c[0] for c in out] == [c[0] for c in bout] and out == T.scaled(bout, exponent)
    assert all(stats[k] == bstats[k] for k in ("passes", "candidates", "moves")) and stats["moves"] >= 1
    assert stats["gain"] == math.ldexp(bstats["gain"], exponent) and 0.0 < stats["gain"] < math.inf


def test_the_other_named_inputs_are_what_they_are_named_for():
    assert T.grid_size(len(M.built("sweep-2178")[0])) == 33
    g, cx, cy = T.cells(list(M.built("clustered-300")[0]))
    assert g == 12 and int(((cx == 0) & (cy == 0)).sum()) >= 200
    assert M.solved("scrambled-400")[5]["passes"] > 100
    for name, key in (("scrambled-400-ring1", 1), ("scrambled-400-ring4", 1), ("scrambled-400-seg1", 2),
                      ("scrambled-400-seg2", 2)):
        assert M.built(name)[key] == int(name[-1]) and M.solved(name)[4] != M.solved("scrambled-400")[4]
    assert M.or_opt(T.scaled(list(M.built("scrambled-400")[0]), 502))[1] == T.RANGE_EDGE[1][1]
