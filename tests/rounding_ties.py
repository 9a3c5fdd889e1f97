"""Tours that tie only after rounding: f64 matrices on which different tours
have different real lengths but the same left fold, because one large edge
absorbs the low bits of the small ones.  A plain helper module: the CPU test
(test_rounding_ties.py) proves what the family is relied on for and tests
K2's host half on it, the GPU test (test_rounding_ties_gpu.py) feeds it to K2,
K1 and K1-wide.

Unlike a lattice, the fold here is NOT exact.  Some tours with fold == optimum
are not DP-consistent (a prefix fold is not the minimum over its city set, yet
rounds to the same next fold), so the reverse-lex least optimal tour is
sometimes not tsp()'s: the certificate has to refuse it, and K1's backtracking
meets steps where members with DIFFERENT table values all satisfy
G[P][m] + d[m][next] == target (the first ascending member wins).

family      construction
outlier     n cities uniform in [0, 2^s)^2, s in -28, -30, -32, -34; city `who`
            (0, n // 2 or n - 1) moved by 2^20 on both axes.  Every tour holds
            two edges of about 2^20.5, whose ulp 2^-32 is of the order of the
            other edges
offset      2^20 + uniform[0, 1) * 2^-31 off the diagonal (non-metric; symmetric
            or not): every entry is 2^20 plus 0, 1 or 2 ulps
scaled      d * 2^k: exact apart from underflow

Everything is deterministic: fixed numpy seeds, listed below where a property
(at least one rounding-tie backtracking step) was asked of them.
"""
import functools
import itertools

import numpy as np

import oracle_py as O

S_VALUES = (-28, -30, -32, -34)
INT_MAX = 2 ** 31 - 1


def left_fold(d, t):
    """tsp.cpp's cost of the closed tour 0, t1..tN, 0 (IEEE double / int)."""
    c = d.dtype.type(0)
    prev = 0
    for x in t:
        c = c + d[prev, x]
        prev = x
    return c + d[prev, 0]


def optimal_set(d):
    """All tours whose left fold equals the optimum (brute force)."""
    n = d.shape[0]
    costs = {}
    for p in itertools.permutations(range(1, n)):
        costs[p] = left_fold(d, p)
    opt = min(costs.values())
    return opt, [p for p, c in costs.items() if c == opt]


def outlier(n, s, who, seed):
    """n - 1 cities in [0, 2^s)^2 and city `who` 2^20 away on both axes -> (n, n) f64."""
    assert who in (0, n // 2, n - 1)
    xy = np.random.default_rng(seed).uniform(0, 1, (n, 2)) * 2.0 ** s
    xy[who] += 2.0 ** 20
    d = O.distance_matrix([(i, xy[i, 0], xy[i, 1]) for i in range(n)])
    assert n * d.max() < INT_MAX
    return d


def offset(n, seed, symmetric):
    """2^20 + uniform * 2^-31 off the diagonal -> (n, n) f64."""
    d = 2.0 ** 20 + np.random.default_rng(seed).uniform(0, 1, (n, n)) * 2.0 ** -31
    if symmetric:
        d = np.triu(d, 1)
        d = d + d.T
    np.fill_diagonal(d, 0.0)
    return np.ascontiguousarray(d)


def scaled(d, k):
    """d * 2^k."""
    return np.ldexp(d, k)


def largest_scale(d):
    """The largest k with n * max(scaled(d, k)) < INT_MAX."""
    n = d.shape[0]
    k = 0
    while n * float(np.ldexp(d.max(), k + 1)) < INT_MAX:
        k += 1
    while n * float(np.ldexp(d.max(), k)) >= INT_MAX:
        k -= 1
    return k


def fold_is_exact(d):
    """The certificate's shortcut condition (search_host.cpp tie_certify): all
    distances multiples of one 2^e and n * max below 2^(e + 53)."""
    nz = d[d != 0.0]
    if nz.size == 0:
        return True
    m, e = np.frexp(nz)                       # nz = m * 2^e, 0.5 <= m < 1 (exact, subnormals too)
    mant = np.ldexp(m, 53).astype(np.int64)   # the 53-bit integer mantissa
    low = (e.astype(np.int64) - 53) + np.array([(int(v) & -int(v)).bit_length() - 1 for v in mant])
    return bool(d.shape[0] * float(nz.max()) < float(np.ldexp(1.0, int(low.min()) + 53)))


def held_karp(d):
    """The reference's DP in plain Python, its fold order and its backtracking
    -> (cost, tour, G) with G[S][k - 1] the table (S over cities 1..N as bits
    0..N-1; None where the reference stores nothing).  Usable to n = 13."""
    n = d.shape[0]
    assert 3 <= n <= 13
    N = n - 1
    dd = [[float(v) for v in row] for row in d]
    full = (1 << N) - 1
    members = [[m for m in range(1, N + 1) if S >> (m - 1) & 1] for S in range(full + 1)]
    G = [None] * (full + 1)
    for S in range(1, full + 1):
        mem = members[S]
        if len(mem) < 2:
            continue
        row = [None] * N
        for k in mem:
            T = S & ~(1 << (k - 1))
            if len(mem) == 2:
                i = members[T][0]
                row[k - 1] = dd[i][k] + dd[0][i]
                continue
            best = float(INT_MAX)
            gt = G[T]
            for m in members[T]:
                cur = gt[m - 1] + dd[m][k]
                if cur < best:
                    best = cur
            row[k - 1] = best
        G[S] = row
    best, best_m = float(INT_MAX), -1
    for m in range(1, N + 1):
        cur = G[full][m - 1] + dd[m][0]
        if cur < best:
            best, best_m = cur, m
    tour = [0] * (n + 1)
    tour[n - 1] = best_m
    S, k, pos = full, best_m, n - 2
    while len(members[S]) > 2:
        T = S & ~(1 << (k - 1))
        pick = next(m for m in members[T] if G[T][m - 1] + dd[m][k] == G[S][k - 1])
        tour[pos] = pick
        pos -= 1
        S, k = T, pick
    tour[pos] = members[S & ~(1 << (k - 1))][0]
    return best, tour, G


def rounding_tie_steps(d, tour, G=None):
    """Backtracking steps along `tour` (the DP's) at which more than one member
    m of P satisfies G[P][m] + d[m][next] == target while those G[P][m] are not
    all the same double: a rounding tie, which the first ascending member wins."""
    n = d.shape[0]
    N = n - 1
    if G is None:
        G = held_karp(d)[2]
    steps = 0
    S = (1 << N) - 1
    for pos in range(n - 1, 2, -1):          # next = tour[pos], chosen from S \ {next}; |S| > 2
        k = tour[pos]
        T = S & ~(1 << (k - 1))
        hit = {G[T][m - 1] for m in range(1, N + 1) if T >> (m - 1) & 1
               and G[T][m - 1] + float(d[m, k]) == G[S][k - 1]}
        steps += len(hit) > 1
        S = T
    return steps


def least_optimal_tour(d, G=None):
    """The reverse-lex least tour whose left fold equals the optimum, without
    enumerating: the device tie rule's winner at sizes brute force cannot reach.

    Rounded addition is monotone, so with the tail t_j..t_N fixed the prefix
    values that fold to the optimum through it form an interval, and no path
    from 0 over the remaining set ending at m folds below that interval (the
    optimum would be lower).  Hence some prefix over P ending at m completes to
    the optimum exactly when the least one, G[P][m], does; the cities are
    chosen from t_N down, the smallest such m each time.  (Checked against
    brute force at n = 8, 9 in test_rounding_ties.py.)"""
    n = d.shape[0]
    N = n - 1
    if G is None:
        G = held_karp(d)[2]
    dd = [[float(v) for v in row] for row in d]
    full = (1 << N) - 1
    opt = min(G[full][m - 1] + dd[m][0] for m in range(1, N + 1))
    tail = []                                  # t_j..t_N, the fixed part

    def completes(v, m):
        prev = m
        for x in tail:
            v = v + dd[prev][x]
            prev = x
        return v + dd[prev][0] == opt

    S = full
    while S & (S - 1):                         # two or more cities left
        pick = next(m for m in range(1, N + 1) if S >> (m - 1) & 1 and completes(G[S][m - 1], m))
        tail.insert(0, pick)
        S &= ~(1 << (pick - 1))
    last = S.bit_length()
    return tuple([last] + tail)


# ---- the instances the tests use------------------------------------------------------------------
#
# Seeds: for every (n, kind) the first seeds 0, 1, 2, ... whose oracle backtracking has at least one
# rounding-tie step (n <= 13; chosen on the reference alone, test_rounding_ties.py checks it).

# (At s = -34 with the outlier at city 0 there is no such step at any seed: every tour starts with
# an edge of about 2^20.5, whose half ulp 2^-33 exceeds the longest other edge, 2^-33.5, so every
# later addition is absorbed and members that reach the target all hold the same double.  Those
# matrices are kept, as heavy ties between equal doubles, and exempt from the step condition.)

# K2 (test_rounding_ties_gpu.py; the host half in test_rounding_ties.py):
# (n, kind, s or symmetric, who, seed).  8 and 9 cities are brute-forced on the CPU.
K2_INSTANCES = (
    (8, "outlier", -28, 0, 8), (8, "outlier", -30, 0, 3), (8, "outlier", -32, 0, 9), (8, "outlier", -32, 4, 1),
    (8, "outlier", -34, 4, 1), (8, "outlier", -34, 4, 0), (8, "outlier", -32, 7, 1), (8, "offset", True, None, 1),
    (8, "offset", False, None, 2),
    (9, "outlier", -28, 0, 1), (9, "outlier", -30, 0, 14), (9, "outlier", -32, 0, 5), (9, "outlier", -32, 4, 1),
    (9, "outlier", -34, 4, 1), (9, "outlier", -34, 4, 2), (9, "outlier", -34, 8, 0), (9, "offset", True, None, 1),
    (9, "offset", False, None, 0),
    (11, "outlier", -28, 0, 3), (11, "outlier", -30, 0, 3), (11, "outlier", -32, 0, 6), (11, "outlier", -34, 5, 0),
    (11, "outlier", -34, 5, 1), (11, "outlier", -32, 10, 0), (11, "offset", True, None, 3),
    (11, "offset", False, None, 5),
    (13, "outlier", -28, 0, 2), (13, "outlier", -30, 0, 2), (13, "outlier", -32, 0, 6), (13, "outlier", -28, 6, 3),
    (13, "outlier", -34, 6, 2), (13, "outlier", -34, 6, 1), (13, "outlier", -30, 12, 3), (13, "offset", True, None, 1),
)

# K1 / ragged / K1-wide: per size 16 distinct matrices, the seeds in k1_kinds' order
K1_SIZES = (5, 9, 12, 13, 14, 15, 16)
K1_SEEDS = {
    5: (3, 3, 9, 0, 6, 2, 1, 0, 14, 2, 7, 15, 30, 1, 21, 7),
    9: (0, 9, 5, 0, 4, 0, 0, 0, 1, 0, 1, 10, 6, 1, 11, 3),
    12: (0, 2, 6, 0, 2, 2, 0, 0, 11, 11, 2, 3, 9, 1, 20, 18),
    13: (0, 2, 6, 0, 2, 2, 0, 0, 1, 17, 2, 3, 9, 1, 5, 19),
    14: (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1),
    15: (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1),
    16: (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1),
}
WIDE_ORACLE_SIZES = (9, 13, 16)   # K1-wide against the oracle: k1_specs(n)
WIDE_K1_SIZES = (18, 20)          # K1-wide against K1: wide_specs(n)
SCALE_SIZES = (9, 13)
SCALES = (-1040, -400, -60, -20, 10, None)  # None: largest_scale(d)


def absorbs_everything(spec):
    """The exempt corner above: outlier at city 0, s = -34."""
    return spec[1] == "outlier" and spec[2] == -34 and spec[3] == 0


def wide_specs(n):
    """10 matrices of 18 or 20 cities: outlier at 0 and n // 2 with every s, offset both ways (seed 0)."""
    return [(n, kind, a, who, 0) for kind, a, who in k1_kinds(n)[:10]]


@functools.lru_cache(maxsize=None)
def scale_base(n, kind):
    """The two ordinary instances the power-of-two scaling starts from: uniform
    points in [0, 1000)^2 and points of the 4 x 4 lattice."""
    rng = np.random.default_rng(8800 + n)
    xy = rng.uniform(0, 1000, (n, 2)) if kind == "uniform" else rng.integers(0, 4, (n, 2)).astype(np.float64)
    d = O.distance_matrix([(i, xy[i, 0], xy[i, 1]) for i in range(n)])
    d.setflags(write=False)
    return d


def scale_cases(n):
    """[(kind, k, scaled matrix)] of a size, every k of SCALES."""
    out = []
    for kind in ("uniform", "lattice"):
        d = scale_base(n, kind)
        for k in SCALES:
            k = largest_scale(d) if k is None else k
            out.append((kind, k, scaled(d, k)))
    return out


def build(spec):
    """(n, "outlier", s, who, seed) or (n, "offset", symmetric, None, seed) -> matrix (read-only, cached)."""
    return _build(*spec)


@functools.lru_cache(maxsize=None)
def _build(n, kind, a, who, seed):
    d = outlier(n, a, who, seed) if kind == "outlier" else offset(n, seed, a)
    d.setflags(write=False)
    return d


def k1_kinds(n):
    """The 16 (kind, s / symmetric, who) of a size: outlier with who in {0, n // 2} and every s, offset both
    ways, then the who = 0 outliers and both offsets once more (another seed)."""
    first = [("outlier", s, who) for who in (0, n // 2) for s in S_VALUES] + [("offset", True, None),
                                                                              ("offset", False, None)]
    again = [("outlier", s, 0) for s in S_VALUES] + [("offset", True, None), ("offset", False, None)]
    return first + again


def k1_specs(n):
    """The 16 instance specs of size n, seeds from K1_SEEDS."""
    return [(n, kind, a, who, seed) for (kind, a, who), seed in zip(k1_kinds(n), K1_SEEDS[n])]


@functools.lru_cache(maxsize=None)
def reference(spec):
    """The oracle's (cost, tour) of an instance, solved once."""
    return O.solve_block(build(spec))
