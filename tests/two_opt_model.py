"""A Python model of the 2-opt stage with a neighbour grid (include/tspgpu.h
"2-opt with a neighbour grid").  TEST INFRASTRUCTURE ONLY;
tests/test_two_opt_model.py checks the model, the GPU tests compare the
library with it bit for bit.

Two statements of the same contract live here.  two_opt() is the one every
test result comes from: it evaluates a pass's candidates as numpy arrays, one
IEEE operation per element and in the contract's order (numpy neither fuses
nor reassociates, and its sqrt is the correctly rounded one).  plain_*() is
the contract word for word in Python floats and math.sqrt, quadratic and
without any neighbour list: a candidate is tested by the definition of N.
The model tests hold the two against each other.

two_opt() lists the neighbours the way the contract describes them
(grid_neighbour_pairs(): cities sorted by cell, an exclusive prefix over the
cell counts, one contiguous run per row), in time near-linear in the number of
pairs; neighbour_pairs() is the L x L definition it is checked against.  Two
hooks of two_opt() (axis_cells, pair_filter) exist for the model tests alone:
they build named WRONG implementations, to show that an input can tell them
from the right one.

Also the named inputs both sides share; every model result is computed once
per process (solved())."""
from __future__ import annotations

import errno
import functools
import math

import numpy as np

import refine_model as R

MAX_GRID = 2048


# ---- the contract's pieces ----

def grid_size(L: int) -> int:
    """The largest g with 2 g g <= L, clamped to [1, 2048]."""
    return max(1, min(MAX_GRID, math.isqrt(L // 2)))


def validate(path) -> int:
    """0, -EINVAL (a non-finite coordinate) or -ERANGE (an extent, or the sum
    of the extents' squares, not finite)."""
    xs = [float(c[1]) for c in path]
    ys = [float(c[2]) for c in path]
    if not all(math.isfinite(v) for v in xs + ys):
        return -errno.EINVAL
    ex, ey = max(xs) - min(xs), max(ys) - min(ys)
    if not (math.isfinite(ex) and math.isfinite(ey) and math.isfinite(ex * ex + ey * ey)):
        return -errno.ERANGE
    return 0


def _axis_cells(v, g: int):
    lo, ext = float(v.min()), float(v.max()) - float(v.min())
    if ext == 0.0:
        return np.zeros(len(v), dtype=np.int64)
    return np.minimum(g - 1, (((v - lo) / ext) * float(g)).astype(np.int64))


def cells(path, axis_cells=None):
    """-> (g, cx, cy): the cell of every city (index in the input).
    axis_cells(v, g) replaces the contract's per-axis formula (mutants only)."""
    axis_cells = axis_cells or _axis_cells
    g = grid_size(len(path))
    x = np.array([c[1] for c in path], dtype=np.float64)
    y = np.array([c[2] for c in path], dtype=np.float64)
    return g, axis_cells(x, g), axis_cells(y, g)


def neighbour_pairs(cx, cy, ring: int, rng=None):
    """Every ordered pair (u, v) of cities with v in N(u), as two arrays; in
    the order `rng` shuffles them into, when given (no result may depend on
    it)."""
    near = (np.abs(cx[:, None] - cx[None, :]) <= ring) & (np.abs(cy[:, None] - cy[None, :]) <= ring)
    u, v = np.nonzero(near)
    if rng is not None:
        k = rng.permutation(len(u))
        u, v = u[k], v[k]
    return u, v


def grid_neighbour_pairs(cx, cy, g: int, ring: int, rng=None):
    """The same set of ordered pairs as neighbour_pairs(), read off the grid
    as the contract describes it: the cities sorted by cell, start[] the
    exclusive prefix over the cell counts, and for each of the 2 ring + 1 rows
    around u the run start[row g + x0] .. start[row g + x1 + 1], x0 and x1
    clamped at the grid's edge, rows outside the grid left out."""
    cx = np.asarray(cx, dtype=np.int64)
    cy = np.asarray(cy, dtype=np.int64)
    cell = cy * g + cx
    by_cell = np.argsort(cell, kind="stable")  # slot -> city
    start = np.concatenate((np.zeros(1, dtype=np.int64), np.cumsum(np.bincount(cell, minlength=g * g))))
    x0, x1 = np.maximum(cx - ring, 0), np.minimum(cx + ring, g - 1)
    us, vs = [], []
    for dy in range(-ring, ring + 1):
        row = cy + dy
        city = np.nonzero((row >= 0) & (row < g))[0]
        s = start[row[city] * g + x0[city]]
        n = start[row[city] * g + x1[city] + 1] - s
        first = np.cumsum(n) - n  # where each city's run begins in this row's list
        us.append(np.repeat(city, n))
        vs.append(by_cell[np.repeat(s - first, n) + np.arange(int(n.sum()), dtype=np.int64)])
    u, v = np.concatenate(us), np.concatenate(vs)
    if rng is not None:
        k = rng.permutation(len(u))
        u, v = u[k], v[k]
    return u, v


def _dist(x, y, a, b):
    dx = x[a] - x[b]
    dy = y[a] - y[b]
    return np.sqrt(dx * dx + dy * dy)


def improving_moves(order, x, y, u, v):
    """Every move with gain > 0 that the pairs reach under `order` (city per
    position): -> (gain, i, j) arrays; a j that both forms reach is listed
    twice."""
    L = len(order)
    pos = np.empty(L, dtype=np.int64)
    pos[order] = np.arange(L)
    # successor form: a = u, c = v; predecessor form: b = u, e = v
    i = np.concatenate((pos[u], pos[u] - 1))
    j = np.concatenate((pos[v], pos[v] - 1))
    ok = (i >= 0) & (j >= i + 2) & (j <= L - 2)
    i, j = i[ok], j[ok]
    a, b, c, e = order[i], order[i + 1], order[j], order[j + 1]
    gain = (_dist(x, y, a, b) + _dist(x, y, c, e)) - (_dist(x, y, a, c) + _dist(x, y, b, e))
    ok = gain > 0.0
    return gain[ok], i[ok], j[ok]


def best_moves(order, x, y, u, v):
    """The best move of every position under `order`: -> (gain, i, j) arrays,
    one entry per position that has one."""
    gain, i, j = improving_moves(order, x, y, u, v)
    k = np.lexsort((j, -gain, i))  # by i, then the largest gain, then the smallest j
    gain, i, j = gain[k], i[k], j[k]
    first = np.ones(len(i), dtype=bool)
    first[1:] = i[1:] != i[:-1]
    return gain[first], i[first], j[first]


def select(gain, i, j, L: int):
    """The greedy selection: by (gain descending, i ascending), a move is
    accepted iff none of its edges i..j belongs to an accepted move."""
    used = np.zeros(L, dtype=bool)
    out = []
    for k in np.lexsort((i, -gain)):
        lo, hi = int(i[k]), int(j[k])
        if not used[lo : hi + 1].any():
            used[lo : hi + 1] = True
            out.append((float(gain[k]), lo, hi))
    return out


def two_opt(path, ring: int = 2, max_passes: int = 1000, rng=None, trace=None, axis_cells=None, pair_filter=None):
    """-> (path, stats), or (None, code) for a refused path.  trace: a list
    that receives each pass's accepted (gain, i, j) list.  The two hooks make
    wrong implementations for the model tests: axis_cells(v, g) replaces the
    per-axis cell formula, pair_filter(u, v, cell) -> a mask of the pairs
    that stay (cell: every city's cell index)."""
    assert 1 <= ring <= 4 and max_passes >= 1 and len(path) >= 1
    code = validate(path)
    if code:
        return None, code
    path = list(path)
    L = len(path)
    stats = {"passes": 0, "candidates": 0, "moves": 0, "gain": 0.0}
    if L < 4:
        return path, stats
    g, cx, cy = cells(path, axis_cells)
    u, v = grid_neighbour_pairs(cx, cy, g, ring, rng)
    if pair_filter is not None:
        keep = pair_filter(u, v, cy * g + cx)
        u, v = u[keep], v[keep]
    x = np.array([c[1] for c in path], dtype=np.float64)
    y = np.array([c[2] for c in path], dtype=np.float64)
    order = np.arange(L)
    while True:
        gain, i, j = best_moves(order, x, y, u, v)
        accepted = select(gain, i, j, L)
        stats["passes"] += 1
        stats["candidates"] += len(gain)
        stats["moves"] += len(accepted)
        for g_k, lo, hi in accepted:
            stats["gain"] = stats["gain"] + g_k
            order[lo + 1 : hi + 1] = order[lo + 1 : hi + 1][::-1].copy()
        if trace is not None:
            trace.append(accepted)
        if not accepted or stats["passes"] == max_passes:
            break
    return [path[int(c)] for c in order], stats


# ---- the contract word for word (quadratic; small inputs and spot checks) ----

def plain_cells(path):
    L = len(path)
    g = grid_size(L)
    out = []
    for axis in (1, 2):
        lo = min(float(c[axis]) for c in path)
        ext = max(float(c[axis]) for c in path) - lo
        out.append([0 if ext == 0.0 else min(g - 1, int(((float(c[axis]) - lo) / ext) * g)) for c in path])
    return out


def plain_d(a, b):
    dx = a[1] - b[1]
    dy = a[2] - b[2]
    return math.sqrt(dx * dx + dy * dy)


def plain_best_moves(path, order, ring: int):
    """path: the input (fixes the grid); order: city per position now.
    -> [(gain, i, j)] of every position that has a best move, by i."""
    L = len(path)
    cx, cy = plain_cells(path)

    def near(s, t):
        return abs(cx[s] - cx[t]) <= ring and abs(cy[s] - cy[t]) <= ring

    out = []
    for i in range(L - 3):
        a, b = order[i], order[i + 1]
        best = None
        for j in range(i + 2, L - 1):
            c, e = order[j], order[j + 1]
            if not (near(a, c) or near(b, e)):
                continue
            gain = (plain_d(path[a], path[b]) + plain_d(path[c], path[e])) - (
                plain_d(path[a], path[c]) + plain_d(path[b], path[e]))
            if gain > 0.0 and (best is None or gain > best[0]):  # (j ascends: an equal gain keeps the smaller j)
                best = (gain, i, j)
        if best:
            out.append(best)
    return out


def plain_two_opt(path, ring: int = 2, max_passes: int = 1000):
    L = len(path)
    stats = {"passes": 0, "candidates": 0, "moves": 0, "gain": 0.0}
    order = list(range(L))
    if L < 4:
        return list(path), stats
    while True:
        cand = sorted(plain_best_moves(path, order, ring), key=lambda m: (-m[0], m[1]))
        accepted = []
        for g_k, i, j in cand:
            if all(j < lo or hi < i for _, lo, hi in accepted):
                accepted.append((g_k, i, j))
        stats["passes"] += 1
        stats["candidates"] += len(cand)
        stats["moves"] += len(accepted)
        for g_k, i, j in accepted:
            stats["gain"] = stats["gain"] + g_k
            order[i + 1 : j + 1] = order[i + 1 : j + 1][::-1]
        if not accepted or stats["passes"] == max_passes:
            break
    return [path[c] for c in order], stats


# ---- the named inputs ----

def zigzag(L: int):
    """L = 4, 5: a line walked 0, L-2, .., 1, L-1; the one move (0, L-2) sorts it."""
    xs = [0] + list(range(L - 2, 0, -1)) + [L - 1]
    return [(10 + k, float(x), 0.5 * x) for k, x in enumerate(xs)]


def bow_tie():
    """Six cities on two rows; the diagonals p1-p2 and p3-p4 cross, and the
    move (1, 3) is the only improving one (tests/test_two_opt_model.py)."""
    pts = [(-1, 0), (0, 0), (1, 1), (1, 0), (0, 1), (-1, 1)]
    return [(20 + k, float(x), float(y)) for k, (x, y) in enumerate(pts)]


BOW_TIE_MOVE = (1, 3)


def one_point(L: int = 50):
    return [(k, 5.0, 5.0) for k in range(L)]


def clustered(seed: int = 4):
    """300 cities in random order, 200 of them inside the grid's cell (0, 0)
    (g = 12 on [0, 1000]^2: cells of 83.3)."""
    rng = np.random.default_rng(seed)
    xy = np.concatenate((rng.uniform(5.0, 80.0, size=(200, 2)), rng.uniform(0.0, 1000.0, size=(98, 2)),
                         np.array([[0.0, 0.0], [1000.0, 1000.0]])))
    xy = xy[rng.permutation(300)]
    return [(k, float(xy[k, 0]), float(xy[k, 1])) for k in range(300)]


def reversed_sweep(L: int = 2000, lo: int = 200, hi: int = 1700, seed: int = 9):
    """A sweep along a gentle curve at irregular spacing with positions
    lo..hi reversed: the move (lo-1, hi) spans more than any workgroup."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(1.0, 9.0, size=L))
    y = 50.0 * np.sin(x / 300.0)
    path = [(k, float(x[k]), float(y[k])) for k in range(L)]
    path[lo : hi + 1] = path[lo : hi + 1][::-1]
    return path


def closed_tour(L: int = 250, seed: int = 21):
    """A scrambled tour that ends on its first city (same id, same place)."""
    path = R.scrambled(L, seed)
    return path + [path[0]]


def sweep(L: int, seed: int, span: float = 1000.0, reversals: int = 40):
    """Uniform cities on [0, span]^2, two of them pinned on the corners, in a
    boustrophedon sweep by grid row (x ascending on even rows, descending on
    odd ones), then `reversals` random sub-ranges of 3 to 49 positions
    reversed: a path that is nearly good at any length, so its passes are few
    and local, with work in every cell of the grid."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, span, size=(L, 2))
    xy[0], xy[1] = (0.0, 0.0), (span, span)
    g = grid_size(L)
    row = np.minimum(g - 1, (xy[:, 1] / span * g).astype(np.int64))
    order = np.lexsort((np.where(row % 2 == 0, xy[:, 0], -xy[:, 0]), row))
    for _ in range(reversals):
        n = int(rng.integers(3, 50))
        s = int(rng.integers(0, L - n + 1))
        order[s : s + n] = order[s : s + n][::-1].copy()
    return [(int(k), float(xy[k, 0]), float(xy[k, 1])) for k in order]


CELL_EDGE_G, CELL_EDGE_EXT = 11, 7.0


def cell_edges(L: int = 242, seed: int = 0):
    """L = 242 (g = 11, no power of two) uniform cities on [0, 7]^2 in random
    order, both extents exactly 7; every third city has each coordinate
    snapped to one of the three doubles around 7 k / 11 (k random in 1..10):
    the cell border itself and its two neighbours, where the rounding of the
    quotient and of the product decides the cell."""
    assert grid_size(L) == CELL_EDGE_G
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, CELL_EDGE_EXT, size=(L, 2))
    xy[0], xy[1] = (0.0, 0.0), (CELL_EDGE_EXT, CELL_EDGE_EXT)
    for c in range(2, L, 3):
        for axis in (0, 1):
            edge = CELL_EDGE_EXT * float(rng.integers(1, CELL_EDGE_G)) / float(CELL_EDGE_G)
            xy[c, axis] = (np.nextafter(edge, -np.inf), edge, np.nextafter(edge, np.inf))[int(rng.integers(0, 3))]
    return [(500 + k, float(xy[k, 0]), float(xy[k, 1])) for k in range(L)]


def scaled(path, exponent: int):
    """Both coordinates times 2^exponent (exact while nothing under- or overflows)."""
    return [(c[0], math.ldexp(c[1], exponent), math.ldexp(c[2], exponent)) for c in path]


def minus_zero_min():
    """bow-tie shifted so that both minima are zero, written as -0.0 on one
    city and as +0.0 on another."""
    path = [(cid, x + 1.0, y) for cid, x, y in bow_tie()]
    assert path[0][1] == 0.0 and path[5][1] == 0.0 and path[1][2] == 0.0 and path[3][2] == 0.0
    path[0] = (path[0][0], -0.0, 0.0)
    path[1] = (path[1][0], path[1][1], -0.0)
    return path


# name -> (builder, ring, max_passes)
IDLE_INPUTS = {
    "L1": (functools.partial(R.scrambled, 1, 1), 2, 1000),
    "L2": (functools.partial(R.scrambled, 2, 2), 2, 1000),
    "L3": (functools.partial(R.scrambled, 3, 3), 2, 1000),
    "one-point-50": (one_point, 2, 1000),
}
MOVING_INPUTS = {
    "L4": (functools.partial(zigzag, 4), 2, 1000),
    "L5": (functools.partial(zigzag, 5), 2, 1000),
    "bow-tie": (bow_tie, 2, 1000),
    "line-300": (functools.partial(R.shuffled_line, 300, 3), 2, 1000),
    "lattice-scrambled-200": (functools.partial(R.lattice_scrambled, 200, 5), 2, 1000),
    "scrambled-400": (functools.partial(R.scrambled, 400, 7), 2, 1000),
    "scrambled-700": (functools.partial(R.scrambled, 700, 8), 2, 1000),
    "clustered-300": (clustered, 2, 1000),
    "reversed-sweep-2000": (reversed_sweep, 2, 1000),
    "closed-tour-251": (closed_tour, 2, 1000),
    "generator-8x64": (R.merged_generator_tour, 2, 1000),
    "scrambled-400-ring1": (functools.partial(R.scrambled, 400, 7), 1, 1000),
    "scrambled-400-ring4": (functools.partial(R.scrambled, 400, 7), 4, 1000),
}
CUT_INPUTS = {
    "scrambled-400-cut1": (functools.partial(R.scrambled, 400, 7), 2, 1),
    "scrambled-400-cut3": (functools.partial(R.scrambled, 400, 7), 2, 3),
}
# Past one workgroup of the grid's scan (1024 cells): the smallest lengths with
# g = 33 (two scan workgroups, the last one ragged), g = 66 (five) and g = 513
# (258 first-level workgroups: two items per lane in the second level).
SWEEP_INPUTS = {
    "sweep-2178": (functools.partial(sweep, 2178, 31), 2, 1000),
    "sweep-8712-ring3": (functools.partial(sweep, 8712, 32), 3, 1000),
    "sweep-526338-ring1-cut3": (functools.partial(sweep, 526338, 33), 1, 3),
}
SCALED_BASE = "scrambled-400"
SCALED_INPUTS = {
    f"{SCALED_BASE}-x2^{e}": (functools.partial(scaled, R.scrambled(400, 7), e), 2, 1000) for e in (500, -500, -520)
}
# (exponent, code): the two neighbours of the -ERANGE limit, SCALED_BASE times 2^exponent
RANGE_EDGE = ((501, 0), (502, -errno.ERANGE))
EDGE_INPUTS = {
    "cell-edges-242": (cell_edges, 1, 1000),
    "minus-zero-min": (minus_zero_min, 2, 1000),
}
SCALE_INPUTS = dict(SWEEP_INPUTS, **SCALED_INPUTS, **EDGE_INPUTS)  # what tests/test_two_opt_scale_gpu.py runs
INPUTS = dict(IDLE_INPUTS, **MOVING_INPUTS, **CUT_INPUTS, **SCALE_INPUTS)


@functools.lru_cache(maxsize=None)
def built(name: str):
    build, ring, passes = INPUTS[name]
    return tuple(build()), ring, passes


@functools.lru_cache(maxsize=None)
def solved(name: str):
    """-> (input path, ring, max_passes, model path, model stats), computed once."""
    path, ring, passes = built(name)
    out, stats = two_opt(list(path), ring, passes)
    return list(path), ring, passes, out, stats
