"""The Python model of the 2-opt stage (tests/two_opt_model.py) against its own
contract, on the CPU.

two_opt() evaluates a pass as numpy arrays; plain_*() is the contract word
for word, quadratic, with no neighbour list.  Here the two are held against
each other, and on every input the GPU tests use the model keeps the cities
and both ends, folds its gain from the left, stops only where no candidate
with gain > 0 is left, does not depend on the order of the neighbour lists,
and APPLIES AT LEAST ONE MOVE and gets strictly shorter under
tspgpu.path_length (so the GPU comparison is not one of untouched paths).
The exceptions are the inputs that exist to move nothing.

The model lists neighbours off a sorted grid (grid_neighbour_pairs); the
L x L definition stays, and the two are held against each other.  The inputs
of tests/test_two_opt_scale_gpu.py are shown to be able to fail: a named wrong
implementation of the model gives another result on each."""
import errno
import math
from fractions import Fraction

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


def test_the_range_limit_lies_between_two_neighbouring_scales():
    """scrambled-400 times 2^501 is the last power of two whose squared
    extents still sum to a finite number; times 2^502 they do not."""
    base = list(T.built(T.SCALED_BASE)[0])
    for e, code in T.RANGE_EDGE:
        path = T.scaled(base, e)
        assert all(math.isfinite(c[1]) and math.isfinite(c[2]) for c in path)
        assert T.validate(path) == code
        out, stats = T.two_opt(path)
        assert (out is None and stats == -errno.ERANGE) if code else stats["moves"] >= 1


# ---- the grid enumeration against the definition ----

OLD_INPUTS = sorted(T.IDLE_INPUTS) + sorted(T.MOVING_INPUTS) + sorted(T.CUT_INPUTS)


def _pair_set(u, v):
    pairs = set(zip(u.tolist(), v.tolist()))
    assert len(pairs) == len(u)  # no pair listed twice
    return pairs


@pytest.mark.parametrize("name", OLD_INPUTS)
def test_grid_enumeration_lists_the_definitions_pairs(name):
    """Sorted cells, exclusive prefix and row runs give the pairs of the L x L
    definition, at every ring; g = 1 and g = 2 (L1 .. L5, bow-tie) have every
    clamp active."""
    path = list(T.built(name)[0])
    g, cx, cy = T.cells(path)
    for ring in (1, 2, 3, 4):
        assert _pair_set(*T.grid_neighbour_pairs(cx, cy, g, ring)) == _pair_set(*T.neighbour_pairs(cx, cy, ring))


def test_grid_sizes_of_the_small_inputs():
    assert [T.grid_size(len(T.built(n)[0])) for n in ("L1", "L3", "L5", "bow-tie", "one-point-50")] == [1, 1, 1, 1, 5]
    assert T.grid_size(8) == 2 and T.grid_size(len(T.built("minus-zero-min")[0])) == 1


# ---- the inputs of tests/test_two_opt_scale_gpu.py: each can fail ----
#
# An input that a wrong kernel would also pass proves nothing.  For every new
# input a named wrong implementation of the model (two_opt()'s hooks) gives
# another (path, stats), or an identity ties the input to one that is checked.

def scan_mutant(first_wrong_cell: int):
    """What a scan that is wrong from cell `first_wrong_cell` on does to the
    row runs, in its mildest form: the cities listed there are not found."""
    return lambda u, v, cell: cell[v] < first_wrong_cell


def test_sweeps_have_the_grids_they_are_named_for():
    want = {"sweep-2178": (33, 2, 1), "sweep-8712-ring3": (66, 5, 1), "sweep-526338-ring1-cut3": (513, 258, 2)}
    for name, (g, workgroups, per_lane) in want.items():
        L = len(T.built(name)[0])
        assert T.grid_size(L) == g and T.grid_size(L - 1) == g - 1  # the smallest such length
        nb = -(-g * g // 1024)
        assert nb == workgroups and -(-nb // 256) == per_lane
        assert (g * g) % 1024 != 0  # a ragged last workgroup
        xs, ys = [c[1] for c in T.built(name)[0]], [c[2] for c in T.built(name)[0]]
        assert (min(xs), max(xs), min(ys), max(ys)) == (0.0, 1000.0, 0.0, 1000.0)


@pytest.mark.parametrize("name", sorted(T.SWEEP_INPUTS))
def test_sweeps_notice_a_scan_wrong_past_its_first_workgroup(name):
    path, ring, passes, out, stats = T.solved(name)
    assert sorted(out) == sorted(path) and out[0] == path[0] and out[-1] == path[-1] and stats["moves"] >= 1
    limits = (1024, 262144) if name == "sweep-526338-ring1-cut3" else (1024,)
    for limit in limits:  # (262144: past the second scan level's first item per lane)
        mout, mstats = T.two_opt(path, ring, passes, pair_filter=scan_mutant(limit))
        assert sorted(mout) == sorted(path)  # a valid path all the same: only the comparison can tell
        assert mout != out and mstats != stats


def test_largest_sweep_is_a_large_pass():
    """Tens of thousands of moves in one pass through the apply kernel's
    search of the prefix array, more than 10^5 candidates through the host
    selection and its copies; cut while it still moves."""
    path, ring, passes, out, stats = T.solved("sweep-526338-ring1-cut3")
    assert stats["passes"] == passes == 3
    assert stats["candidates"] > 100000 and stats["moves"] > 30000
    trace = []
    T.two_opt(path, ring, 1, trace=trace)
    assert len(trace[0]) > 10000


@pytest.mark.parametrize("name", ["sweep-2178", "sweep-8712-ring3"])
def test_converging_sweeps_stop_by_the_rule(name):
    path, ring, passes, out, stats = T.solved(name)
    trace = []
    again, stats2 = T.two_opt(path, ring, passes, trace=trace)
    assert again == out and stats2 == stats
    assert stats["passes"] == len(trace) < passes and not trace[-1] and stats["passes"] > 3
    assert tspgpu.path_length(out) < tspgpu.path_length(path)
    if len(path) <= 3000:  # re-enumerated by the definition, no candidate with gain > 0 is left
        assert T.plain_best_moves(path, _order_of(path, out), ring) == []
    else:  # (quadratic: out of reach) the model's own last pass, from its result
        _, stats3 = T.two_opt(out, ring, 1)
        assert stats3 == {"passes": 1, "candidates": 0, "moves": 0, "gain": 0.0}


def test_ring_three_differs_from_ring_two():
    path, ring, passes, out, stats = T.solved("sweep-8712-ring3")
    assert ring == 3
    out2, stats2 = T.two_opt(path, 2, passes)
    assert out2 != out and stats2 != stats


def product_first(v, g):
    """((v - lo) * g) / ext in place of ((v - lo) / ext) * g."""
    lo, ext = float(v.min()), float(v.max()) - float(v.min())
    return np.minimum(g - 1, (((v - lo) * float(g)) / ext).astype(np.int64))


def _fma(a: float, b: float, c: float) -> float:
    """a b + c rounded once (Fraction -> float rounds to nearest even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def reciprocal_fused(v, g):
    """The division as a product with 1 / ext, the subtraction fused into it:
    fma(v, r, -(lo r)) * g."""
    lo, ext = float(v.min()), float(v.max()) - float(v.min())
    r = 1.0 / ext
    q = np.array([_fma(float(t), r, -(lo * r)) for t in v])
    return np.minimum(g - 1, (q * float(g)).astype(np.int64))


def product_unrounded(v, g):
    """The contract's quotient, but its product with g truncated without
    having been rounded (as when it is fused into what follows)."""
    lo, ext = float(v.min()), float(v.max()) - float(v.min())
    q = (v - lo) / ext
    return np.minimum(g - 1, np.array([int(Fraction(float(t)) * g) for t in q], dtype=np.int64))


@pytest.mark.parametrize("mutant", [product_first, reciprocal_fused, product_unrounded])
def test_cell_edges_notice_another_rounding_of_the_cell_formula(mutant):
    path, ring, passes, out, stats = T.solved("cell-edges-242")
    g, cx, cy = T.cells(path)
    assert g == T.CELL_EDGE_G and ring == 1
    xs, ys = [c[1] for c in path], [c[2] for c in path]
    assert (min(xs), max(xs), min(ys), max(ys)) == (0.0, T.CELL_EDGE_EXT, 0.0, T.CELL_EDGE_EXT)
    _, mx, my = T.cells(path, mutant)
    assert int((mx != cx).sum() + (my != cy).sum()) >= 5  # coordinates that change their cell
    mout, mstats = T.two_opt(path, ring, passes, axis_cells=mutant)
    assert mout != out and mstats != stats


def test_cell_edges_equal_the_plain_statement():
    path, ring, passes, out, stats = T.solved("cell-edges-242")
    assert [T.cells(path)[1].tolist(), T.cells(path)[2].tolist()] == T.plain_cells(path)
    pout, pstats = T.plain_two_opt(path, ring, passes)
    assert pout == out and pstats == stats and stats["moves"] >= 1


def test_minus_zero_minimum_is_the_bow_tie():
    path, ring, passes, out, stats = T.solved("minus-zero-min")
    signs = lambda axis: sorted(math.copysign(1.0, c[axis]) for c in path if c[axis] == 0.0)
    assert signs(1) == [-1.0, 1.0] and signs(2) == [-1.0, 1.0, 1.0]
    _, _, _, bout, bstats = T.solved("bow-tie")
    assert [c[0] for c in out] == [c[0] for c in bout] and stats == bstats and stats["moves"] == 1
    assert T.plain_two_opt(path, ring, passes) == (out, stats)
    # the zeros keep their signs through the move
    assert all(math.copysign(1.0, a[k]) == math.copysign(1.0, b[k]) for a in out for b in path if a[0] == b[0]
               for k in (1, 2))


@pytest.mark.parametrize("exponent", [500, -500, -520])
def test_scaled_inputs_are_the_base_input_times_a_power_of_two(exponent):
    """Same order, passes, candidates and moves as scrambled-400 and its gain
    times the scale exactly: a mismatch on the GPU is the distance code's."""
    _, _, _, bout, bstats = T.solved(T.SCALED_BASE)
    path, ring, passes, out, stats = T.solved(f"{T.SCALED_BASE}-x2^{exponent}")
    assert T.validate(path) == 0
    assert [c[0] for c in out] == [c[0] for c in bout] and out == T.scaled(bout, exponent)
    assert all(stats[k] == bstats[k] for k in ("passes", "candidates", "moves")) and stats["moves"] >= 1
    assert stats["gain"] == math.ldexp(bstats["gain"], exponent) and 0.0 < stats["gain"] < math.inf
    x = np.array([c[1] for c in path])
    y = np.array([c[2] for c in path])
    sq = np.square(x[:-1] - x[1:]) + np.square(y[:-1] - y[1:])  # the input's own edges
    if exponent == 500:
        ex, ey = x.max() - x.min(), y.max() - y.min()
        assert 1.0e307 < ex * ex + ey * ey < math.inf and sq.max() > 2.0**1015
    if exponent == -500:
        assert sq.max() < 2.0**-900 and sq.min() >= 2.0**-1022  # the scaled branch, all normal
    if exponent == -520:
        tiny = np.finfo(np.float64).tiny
        assert (np.square(x[:-1] - x[1:]) < tiny).any() and (sq >= tiny).any()  # subnormal squares and normal sums


def _tied_positions(name):
    """The positions whose largest gain under the input order is reached at
    two or more j, and the first pass's candidates' gains."""
    path, ring, _ = T.built(name)
    path = list(path)
    g, cx, cy = T.cells(path)
    u, v = T.grid_neighbour_pairs(cx, cy, g, ring)
    x = np.array([c[1] for c in path])
    y = np.array([c[2] for c in path])
    order = np.arange(len(path))
    best = {}
    for gain, i, j in set(zip(*(a.tolist() for a in T.improving_moves(order, x, y, u, v)))):
        top = best.setdefault(i, [gain, set()])
        if gain > top[0]:
            top[0], top[1] = gain, {j}
        elif gain == top[0]:
            top[1].add(j)
    return sum(len(js) >= 2 for _, js in best.values()), T.best_moves(order, x, y, u, v)[0]


def test_the_tie_inputs_tie():
    """lattice-scrambled-200 and line-300 are where "the smallest j on equal
    gains" and "i ascending on equal gains" decide."""
    lattice, gains = _tied_positions("lattice-scrambled-200")
    line, _ = _tied_positions("line-300")
    assert lattice >= 10 and line >= 10
    assert len(gains) - len(set(gains.tolist())) >= 20  # candidates whose gain another position has too
