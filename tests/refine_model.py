"""A Python model of the fixed-end path problem and the window refinement
(include/tspgpu.h "Fixed-end shortest paths and the window refinement"), on the
CPU oracle alone: oracle_py.distance_matrix for a window's matrix,
oracle_py.solve_block on the folded matrix for its answer.  TEST
INFRASTRUCTURE ONLY; tests/test_refine_model.py checks the model, the GPU
tests compare the library with it bit for bit.

Also the input builders both sides share.  Every refinement input the GPU tests
use is named in REFINE_INPUTS, and its model result is computed once per
process (refined())."""
from __future__ import annotations

import errno
import functools
import itertools
import math

import numpy as np

import oracle_py as O

INT_MAX = 2**31 - 1
MAX_W = 20


# ---- the path problem ----

def fold_matrix(D):
    """The (w-1) x (w-1) matrix K1 is given: P[i][j] = D[i][j] for j >= 1,
    P[i][0] = D[i][w-1] for i >= 1, P[0][0] = 0."""
    D = np.asarray(D)
    w = D.shape[0]
    P = D[: w - 1, : w - 1].copy()
    P[1:, 0] = D[1 : w - 1, w - 1]
    P[0, 0] = 0
    return P


def validate(P) -> int:
    """tspgpu_validate / tspgpu_validate_i32 on one matrix."""
    P = np.asarray(P)
    n = P.shape[0]
    if P.dtype.kind == "f":
        if not np.isfinite(P).all() or (P < 0).any() or np.signbit(P).any():
            return -errno.EINVAL
    elif (P < 0).any():
        return -errno.EINVAL
    if float(n) * float(P.max()) >= float(INT_MAX):
        return -errno.ERANGE
    return 0


def solve_path(D):
    """-> (cost, order [0, t1..tm, w-1], status); a bad block: (nan, [-1]*w, code)."""
    D = np.asarray(D)
    w = D.shape[0]
    P = fold_matrix(D)
    st = validate(P)
    if st:
        return math.nan, [-1] * w, st
    cost, tour = O.solve_block(P.astype(np.float64))
    assert len(tour) == w and tour[0] == 0 and tour[-1] == 0
    return cost, tour[:-1] + [w - 1], 0


def left_fold(D, order):
    s = D[order[0]][order[1]]
    for a, b in zip(order[1:-1], order[2:]):
        s = s + D[a][b]
    return s


def brute_force(D):
    """The minimum left fold over every interior permutation (w <= 9)."""
    D = np.asarray(D, dtype=np.float64).tolist()  # (Python floats: the same IEEE adds, faster to index)
    w = len(D)
    return min(float(left_fold(D, (0,) + p + (w - 1,))) for p in itertools.permutations(range(1, w - 1)))


# ---- the refinement ----

def pass_windows(L: int, m: int, p: int):
    """(offset, W) of pass p."""
    o = (m + 1) // 2 if p % 2 else 0
    return o, max(0, (L - 1 - o) // (m + 1))


def refine(path, m: int, max_passes: int, trace=None):
    """-> (path, stats): the contract, window by window.  trace: a list that
    receives (pass, k, old, new, status, replaced) per window."""
    assert max_passes >= 1 and 2 <= m <= MAX_W - 2 and len(path) >= 2
    path = list(path)
    L = len(path)
    stats = {"passes": 0, "windows": 0, "replaced": 0, "skipped": 0, "gain": 0.0}
    if pass_windows(L, m, 0)[1] == 0:
        return path, stats
    cache = {}
    before = 0
    p = 0
    while True:
        o, W = pass_windows(L, m, p)
        src = list(path)  # (windows share only fixed ends: order within a pass is free)
        replaced = 0
        for k in range(W):
            s = o + k * (m + 1)
            win = src[s : s + m + 2]
            key = tuple((x, y) for _, x, y in win)
            if key not in cache:
                D = O.distance_matrix(win)
                idn = list(range(m + 2))
                cache[key] = (float(left_fold(D, idn)),) + solve_path(D)
            old, new, order, st = cache[key]
            stats["windows"] += 1
            take = st == 0 and new < old
            if st != 0:
                stats["skipped"] += 1
            if take:
                path[s + 1 : s + m + 1] = [win[t] for t in order[1:-1]]
                replaced += 1
                stats["gain"] = stats["gain"] + (old - new)
            if trace is not None:
                trace.append((p, k, old, new, st, take))
        stats["replaced"] += replaced
        stats["passes"] = p + 1
        if p + 1 == max_passes or (p >= 1 and replaced == 0 and before == 0):
            break
        before = replaced
        p += 1
    return path, stats


def path_length(path) -> float:
    """The left fold of the oracle's distance on consecutive cities."""
    s = 0.0
    for a, b in zip(path[:-1], path[1:]):
        s = s + float(O.distance_matrix([a, b])[0][1])
    return s


# ---- input builders ----

def scrambled(L: int, seed: int, span: float = 1000.0):
    """L uniform cities in random order."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, span, size=(L, 2))
    return [(1000 + i, float(xy[i, 0]), float(xy[i, 1])) for i in range(L)]


def shuffled_line(L: int, seed: int):
    """Cities on a line at irregular spacing, visited in shuffled order."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(1.0, 9.0, size=L))
    order = rng.permutation(L)
    return [(int(i), float(x[i]), 0.25 * float(x[i])) for i in order]


def lattice_scrambled(L: int, seed: int, side: int = 6):
    """Integer lattice points with coincident cities, in random order."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, side, size=(L, 2))
    return [(i, float(xy[i, 0]), float(xy[i, 1])) for i in range(L)]


def lattice_ties(L: int):
    """A monotone walk along a lattice line, every point visited twice in a
    row: the given order is optimal in every window (sums of small integers
    are exact), other orders only tie with it, so nothing may be replaced."""
    return [(i, float(i // 2), 3.0) for i in range(L)]


def with_outlier(L: int, seed: int, at: int):
    """scrambled(L) with city `at` moved 10^9 away: its windows are -ERANGE."""
    path = scrambled(L, seed)
    cid, x, y = path[at]
    path[at] = (cid, x + 1.0e9, y)
    return path


def merged_generator_tour(n: int = 8, B: int = 64, X: int = 1000, Y: int = 1000):
    """The reference's merged tour of ./tsp n B X Y on one rank: every block
    solved, then folded from the left with mergeBlocks (all on the oracle)."""
    acc = None
    for blk in O.generate(n, B, X, Y):
        c, t = O.solve_block(O.distance_matrix(blk))
        sol = ([blk[i] for i in t], c)
        acc = sol if acc is None else O.merge_blocks(acc[0], acc[1], sol[0], sol[1])
    return acc[0]


# name -> (builder, m, max_passes); what tests/test_refine_gpu.py runs.  Every
# input but the tie-only lattice replaces at least one window in the model
# (tests/test_refine_model.py asserts it).
def first_replacing(L: int, m: int, max_passes: int, seed: int):
    """scrambled(L, s) for the first seed s >= seed whose model run replaces a
    window (a path with a single short window is sometimes optimal as drawn);
    a path too short for a window is taken as it comes."""
    while True:
        path = scrambled(L, seed)
        if L < m + 2 or refine(path, m, max_passes)[1]["replaced"]:
            return path
        seed += 1


def _small_cases():
    out = {}
    for m in (2, 3, 7):
        for tag, L in (("2", 2), ("m+1", m + 1), ("m+2", m + 2), ("m+3", m + 3), ("2(m+1)", 2 * (m + 1)),
                       ("2(m+1)+1", 2 * (m + 1) + 1), ("5(m+1)+m/2", 5 * (m + 1) + m // 2)):
            out[f"small-m{m}-L{tag}"] = (functools.partial(first_replacing, L, m, 6, 100 * m + L), m, 6)
    return out


SMALL_INPUTS = _small_cases()
REFINE_INPUTS = {
    "scrambled-400-m7": (functools.partial(scrambled, 400, 7), 7, 8),
    "scrambled-600-m15": (functools.partial(scrambled, 600, 15), 15, 4),
    "line-300-m7": (functools.partial(shuffled_line, 300, 3), 7, 8),
    "lattice-scrambled-200-m7": (functools.partial(lattice_scrambled, 200, 5), 7, 8),
    "outlier-200-m7": (functools.partial(with_outlier, 200, 11, 77), 7, 8),
    "generator-8x64-m15": (merged_generator_tour, 15, 8),
}
TIE_INPUT = ("lattice-ties-120-m7", functools.partial(lattice_ties, 120), 7, 8)


def wide_input(cus: int):
    """m = 12 with CUs + 3 windows in pass 0: K1's large-batch variant runs."""
    return scrambled(13 * (cus + 3) + 1, 12), 12, 2


@functools.lru_cache(maxsize=None)
def built(name: str):
    table = dict(REFINE_INPUTS, **SMALL_INPUTS, **{TIE_INPUT[0]: TIE_INPUT[1:]})
    build, m, passes = table[name]
    return tuple(build()), m, passes


@functools.lru_cache(maxsize=None)
def refined(name: str):
    """-> (input path, m, max_passes, model path, model stats), computed once."""
    path, m, passes = built(name)
    out, stats = refine(list(path), m, passes)
    return list(path), m, passes, out, stats
