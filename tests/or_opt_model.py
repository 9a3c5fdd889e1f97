"""A Python model of the Or-opt stage with a neighbour grid (include/tspgpu.h
"Or-opt with a neighbour grid").  TEST INFRASTRUCTURE ONLY;
tests/test_or_opt_model.py checks the model, the GPU tests compare the library
with it bit for bit.

The grid, the neighbour pairs, the validation and most inputs are the 2-opt
model's (tests/two_opt_model.py).  As there, two statements of the contract
live here: or_opt() evaluates a pass's candidates as numpy arrays, one IEEE
operation per element in the contract's order; plain_or_opt() is the contract
word for word in Python floats, with N tested by its definition.

A move is the tuple (a, k, t, rev): positions a..a+k-1 go into edge t, as they
lie or reversed.  or_opt() takes one hook, `mutant`, for the model tests
alone: a name out of MUTANTS builds a WRONG implementation, to show that an
input can tell it from the right one.

Every model result is computed once per process (solved())."""
from __future__ import annotations

import functools
import math

import numpy as np

import refine_model as R
import two_opt_model as T

MUTANTS = ("no-trailing", "no-reversed", "ties-largest", "wide-exclusion")


# ---- the contract's pieces ----

def move_range(a: int, k: int, t: int):
    """The edge range [lo, hi] of a move: positions lo+1..hi are rotated."""
    h = a + k - 1
    return (a - 1, t) if t > h else (t, h)


def apply_move(order, a: int, k: int, t: int, rev: int):
    """The order (a list or an array) with one move applied, in place."""
    h = a + k - 1
    seg = list(order[a : h + 1])
    if rev:
        seg.reverse()
    if t > h:
        order[a : t + 1] = list(order[h + 1 : t + 1]) + seg
    else:
        order[t + 1 : h + 1] = seg + list(order[t + 1 : a])


def segment_kinds(max_seg: int, mutant=None):
    """(lead, k): the segment of k positions that has position s at its first
    (lead) or its last end; k = 1 counts once."""
    kinds = [(True, k) for k in range(1, max_seg + 1)]
    if mutant != "no-trailing":
        kinds += [(False, k) for k in range(2, max_seg + 1)]
    return kinds


def _dist(x, y, a, b):
    dx = x[a] - x[b]
    dy = y[a] - y[b]
    return np.sqrt(dx * dx + dy * dy)


def improving_moves(order, x, y, u, v, max_seg: int, mutant=None):
    """Every move with gain > 0 that the pairs (u, v in N(u)) reach under
    `order`: -> (gain, s, a, k, t, rev) arrays; a move reached twice is listed
    twice."""
    L = len(order)
    pos = np.empty(L, dtype=np.int64)
    pos[order] = np.arange(L)
    keep = u != v
    s0, q0 = pos[u[keep]], pos[v[keep]]
    keep = (s0 >= 1) & (s0 <= L - 2)
    s0, q0 = s0[keep], q0[keep]
    out = []
    for lead, k in segment_kinds(max_seg, mutant):
        a0 = s0 if lead else s0 - (k - 1)
        for side in (0, 1):  # 0: t = q, f follows v; 1: t = q - 1, f precedes v
            rev = 0 if k == 1 else int(lead == bool(side))
            if rev and mutant == "no-reversed":
                continue
            t = q0 - side
            h = a0 + (k - 1)
            ok = (a0 >= 1) & (h <= L - 2) & (t >= 0) & (t <= L - 2) & ((t < a0 - 1) | (t > h))
            if mutant == "wide-exclusion":
                ok &= (t != a0 - 2) & (t != h + 1)
            s, a, t, h = s0[ok], a0[ok], t[ok], h[ok]
            first, last, P, N, c, e = order[a], order[h], order[a - 1], order[h + 1], order[t], order[t + 1]
            xx, yy = (last, first) if rev else (first, last)
            gain = ((_dist(x, y, P, first) + _dist(x, y, last, N)) + _dist(x, y, c, e)) - (
                (_dist(x, y, P, N) + _dist(x, y, c, xx)) + _dist(x, y, yy, e))
            ok = gain > 0.0
            n = int(ok.sum())
            out.append((gain[ok], s[ok], a[ok], np.full(n, k, dtype=np.int64), t[ok], np.full(n, rev, dtype=np.int64)))
    return tuple(np.concatenate(col) for col in zip(*out))


def best_moves(order, x, y, u, v, max_seg: int, mutant=None):
    """The best move of every position: the largest gain, on equal gains the
    lexicographically smallest (a, k, t, rev) -> the six arrays, one entry per
    position that has a move."""
    gain, s, a, k, t, rev = improving_moves(order, x, y, u, v, max_seg, mutant)
    sign = -1 if mutant == "ties-largest" else 1
    idx = np.lexsort((sign * rev, sign * t, sign * k, sign * a, -gain, s))
    gain, s, a, k, t, rev = (col[idx] for col in (gain, s, a, k, t, rev))
    first = np.ones(len(s), dtype=bool)
    first[1:] = s[1:] != s[:-1]
    return tuple(col[first] for col in (gain, s, a, k, t, rev))


def select(gain, s, a, k, t, rev, L: int):
    """The greedy selection: by (gain descending, s ascending), a move is
    accepted iff none of its edges lo..hi belongs to an accepted move."""
    used = np.zeros(L, dtype=bool)
    out = []
    for n in np.lexsort((s, -gain)):
        lo, hi = move_range(int(a[n]), int(k[n]), int(t[n]))
        if not used[lo : hi + 1].any():
            used[lo : hi + 1] = True
            out.append((float(gain[n]), int(s[n]), int(a[n]), int(k[n]), int(t[n]), int(rev[n])))
    return out


def or_opt(path, ring: int = 2, max_seg: int = 3, max_passes: int = 1000, rng=None, trace=None, mutant=None):
    """-> (path, stats), or (None, code) for a refused path.  trace: a list
    that receives each pass's accepted (gain, s, a, k, t, rev) list.  rng
    shuffles the pair list (no result may depend on its order)."""
    assert 1 <= ring <= 4 and 1 <= max_seg <= 3 and max_passes >= 1 and len(path) >= 1
    assert mutant is None or mutant in MUTANTS
    code = T.validate(path)
    if code:
        return None, code
    path = list(path)
    L = len(path)
    stats = {"passes": 0, "candidates": 0, "moves": 0, "gain": 0.0}
    if L < 4:
        return path, stats
    g, cx, cy = T.cells(path)
    u, v = T.grid_neighbour_pairs(cx, cy, g, ring, rng)
    x = np.array([c[1] for c in path], dtype=np.float64)
    y = np.array([c[2] for c in path], dtype=np.float64)
    order = np.arange(L)
    while True:
        best = best_moves(order, x, y, u, v, max_seg, mutant)
        accepted = select(*best, L)
        stats["passes"] += 1
        stats["candidates"] += len(best[0])
        stats["moves"] += len(accepted)
        for g_k, _, a, k, t, rev in accepted:  # (disjoint ranges: one after the other is all at once)
            stats["gain"] = stats["gain"] + g_k
            apply_move(order, a, k, t, rev)
        if trace is not None:
            trace.append(accepted)
        if not accepted or stats["passes"] == max_passes:
            break
    return [path[int(c)] for c in order], stats


# ---- the contract word for word (quadratic; small inputs and spot checks) ----

def plain_best_moves(path, order, ring: int, max_seg: int):
    """path: the input (fixes the grid); order: city per position now.
    -> [(gain, s, a, k, t, rev)] of every position that has a best move, by s."""
    L = len(path)
    cx, cy = T.plain_cells(path)
    near = [[w for w in range(L) if abs(cx[f] - cx[w]) <= ring and abs(cy[f] - cy[w]) <= ring] for f in range(L)]
    pos = [0] * L
    for p, c in enumerate(order):
        pos[c] = p
    d = lambda s, t: T.plain_d(path[s], path[t])
    out = []
    for s in range(1, L - 1):
        f = order[s]
        segments = {(s, k) for k in range(1, max_seg + 1)} | {(s - k + 1, k) for k in range(1, max_seg + 1)}
        moves = set()
        for a, k in segments:
            h = a + k - 1
            if a < 1 or h > L - 2:
                continue
            for w in near[f]:
                if w == f:
                    continue
                q = pos[w]
                # t = q: f follows v, so f is x; t = q - 1: f precedes v, so f is y
                for t, f_is_x in ((q, True), (q - 1, False)):
                    if t < 0 or t > L - 2 or a - 1 <= t <= h:
                        continue
                    if k == 1:
                        rev = 0
                    elif f_is_x:
                        rev = 0 if s == a else 1  # x = first as it lies, x = last reversed
                    else:
                        rev = 0 if s == h else 1  # y = last as it lies, y = first reversed
                    moves.add((a, k, t, rev))
        best = None
        for a, k, t, rev in sorted(moves):  # (ascending tuples: an equal gain keeps the smaller one)
            h = a + k - 1
            first, last, P, N, c, e = order[a], order[h], order[a - 1], order[h + 1], order[t], order[t + 1]
            xx, yy = (last, first) if rev else (first, last)
            gain = ((d(P, first) + d(last, N)) + d(c, e)) - ((d(P, N) + d(c, xx)) + d(yy, e))
            if gain > 0.0 and (best is None or gain > best[0]):
                best = (gain, s, a, k, t, rev)
        if best:
            out.append(best)
    return out


def plain_or_opt(path, ring: int = 2, max_seg: int = 3, max_passes: int = 1000):
    L = len(path)
    stats = {"passes": 0, "candidates": 0, "moves": 0, "gain": 0.0}
    order = list(range(L))
    if L < 4:
        return list(path), stats
    while True:
        cand = sorted(plain_best_moves(path, order, ring, max_seg), key=lambda m: (-m[0], m[1]))
        accepted, ranges = [], []
        for m in cand:
            lo, hi = move_range(*m[2:5])
            if all(hi < l2 or h2 < lo for l2, h2 in ranges):
                accepted.append(m)
                ranges.append((lo, hi))
        stats["passes"] += 1
        stats["candidates"] += len(cand)
        stats["moves"] += len(accepted)
        for g_k, _, a, k, t, rev in accepted:
            stats["gain"] = stats["gain"] + g_k
            apply_move(order, a, k, t, rev)
        if not accepted or stats["passes"] == max_passes:
            break
    return [path[c] for c in order], stats


# ---- the named inputs ----

def on_a_line(ts, first_id: int):
    """Cities at t (3, 4): every distance is 5 |dt| exactly, so equal moves tie
    exactly and the tie rules decide."""
    return [(first_id + n, 3.0 * t, 4.0 * t) for n, t in enumerate(ts)]


# The smallest paths with a move, one per segment length, each touching both
# fixed ends.  Inside 2..4 movable positions a move of k cities past j others
# is also a move of the j past the k, with the same gain: the model's order
# decides which of the equal moves a pass accepts (FIRST_MOVES below; the model
# tests check that the move the input is named for is among the candidates).
SMALL = {
    "L4": (0, 2, 1, 3),        # k = 1: position 1 into edge 2
    "L5": (0, 2, 3, 1, 4),     # k = 2: positions 1..2 into edge L-2 = 3
    "L6": (0, 4, 3, 2, 1, 5),  # k = 3: positions 2..4 reversed into edge 0
}
NAMED_MOVES = {"L4": (1, 1, 2, 0), "L5": (1, 2, 3, 0), "L6": (2, 3, 0, 1)}


def curve(L: int = 2000, seed: int = 9):
    """two_opt_model.reversed_sweep()'s curve, in order."""
    return T.reversed_sweep(L, 1, 1, seed)


def stray(direction: int, count: int = 1, near: int = 200, far: int = 1800):
    """The curve with `count` cities about 1600 positions from where they
    belong, in reversed order among themselves when there are several: the
    repair is one rotation of about 1600 positions, larger than any workgroup.
    direction +1: the cities of positions far.. sit at near.. and move
    forward (t > h); -1: those of near.. sit at far.. and move backward."""
    path = curve()
    src, dst = (far, near) if direction > 0 else (near, far)
    seg = path[src : src + count][::-1]
    del path[src : src + count]
    at = dst if dst < src else dst - count
    path[at:at] = seg
    return path


def two_opt_optimal(name: str):
    """The 2-opt model's result on its input `name`: nothing left for 2-opt."""
    return list(T.solved(name)[3])


TWO_OPT_OPTIMAL = ("scrambled-400", "scrambled-700", "clustered-300", "generator-8x64", "closed-tour-251")

# name -> (builder, ring, max_seg, max_passes)
IDLE_INPUTS = {name: (T.IDLE_INPUTS[name][0], 2, 3, 1000) for name in ("L1", "L2", "L3", "one-point-50")}
SMALL_INPUTS = {name: (functools.partial(on_a_line, ts, 10 * len(ts)), 2, 3, 1000) for name, ts in SMALL.items()}
STRAY_INPUTS = {
    "stray-forward-2000": (functools.partial(stray, 1), 2, 3, 1000),
    "stray-backward-2000": (functools.partial(stray, -1), 2, 3, 1000),
    "stray-three-reversed-2000": (functools.partial(stray, 1, 3), 2, 3, 1000),
}
OPTIMAL_INPUTS = {f"2opt:{name}": (functools.partial(two_opt_optimal, name), 2, 3, 1000) for name in TWO_OPT_OPTIMAL}
scrambled_400 = functools.partial(R.scrambled, 400, 7)
MOVING_INPUTS = dict(SMALL_INPUTS, **STRAY_INPUTS, **OPTIMAL_INPUTS, **{
    "lattice-scrambled-200": (functools.partial(R.lattice_scrambled, 200, 5), 2, 3, 1000),
    "scrambled-400": (scrambled_400, 2, 3, 1000),
    "clustered-300": (T.clustered, 2, 3, 1000),
    "sweep-2178": (functools.partial(T.sweep, 2178, 31), 2, 3, 1000),
    "scrambled-400-ring1": (scrambled_400, 1, 3, 1000),
    "scrambled-400-ring4": (scrambled_400, 4, 3, 1000),
    "scrambled-400-seg1": (scrambled_400, 2, 1, 1000),
    "scrambled-400-seg2": (scrambled_400, 2, 2, 1000),
})
CUT_INPUTS = {
    "scrambled-400-cut1": (scrambled_400, 2, 3, 1),
    "scrambled-400-cut3": (scrambled_400, 2, 3, 3),
}
SCALED_BASE = "scrambled-400"
SCALED_INPUTS = {
    f"{SCALED_BASE}-x2^{e}": (functools.partial(T.scaled, R.scrambled(400, 7), e), 2, 3, 1000) for e in (500, -500)
}
INPUTS = dict(IDLE_INPUTS, **MOVING_INPUTS, **CUT_INPUTS, **SCALED_INPUTS)


@functools.lru_cache(maxsize=None)
def built(name: str):
    build, ring, max_seg, passes = INPUTS[name]
    return tuple(build()), ring, max_seg, passes


@functools.lru_cache(maxsize=None)
def solved(name: str):
    """-> (input path, ring, max_seg, max_passes, model path, model stats), computed once."""
    path, ring, max_seg, passes = built(name)
    out, stats = or_opt(list(path), ring, max_seg, passes)
    return list(path), ring, max_seg, passes, out, stats
