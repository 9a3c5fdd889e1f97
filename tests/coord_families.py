"""Coordinate families for the distance build (csrc/cities.hip, dist_exact.h)
and K3 (csrc/merge.hip, paths.hip): the reference generator's cities
(bench.Shard) moved off the generator's [0, 1000) plane, plus a few built
point sets, and the K3 inputs made from them.  A plain helper module: the CPU
test (test_coord_families.py) proves what every family claims, the GPU tests
(test_cities_edges_gpu.py, test_merge_edges_gpu.py) feed them to the kernels.

Everything is deterministic: fixed numpy seeds, the generator's srand(0)
stream, no rand().

family      construction
neg         block k even: (x - 500, y - 500); k odd: (-x, -y); city 0 of block 0 has x = -0.0
shift40     x + 2^40, y + 2^40: coordinates snap to a 2^-12 grid (many exact ties)
shift52     x + 2^52, y + 2^52: the integer grid (coincident cities)
scale<k>    ldexp(x, k), ldexp(y, k) for k in -400, -40, 20, 400 (and 17, for the solves alone)
cut_low     scale -450: squares on both sides of 2^-900
cut_high    scale 495: squares on both sides of 2^1000
under       scale -540: every square subnormal or zero
sub         scale -1030: coordinates subnormal or just above, every square zero
over        scale 507: some squares infinite, some finite
mixed       every city its own ldexp(., e), e in [-300, 300], x and y independently
midpoint    city 0 at the origin, city k at an odd integer x in [94906267, 134217727]
            (x*x lies exactly halfway between two doubles), y a multiple of 0.25
few_bits    integers and quarter-integers in [-512, 512]: every square exact
special     every third block mixes +inf, -inf, nan and -0.0 into ordinary cities
"""
import functools
import math

import numpy as np

import tspgpu
from bench import Shard

LOW, HIGH = 2.0 ** -900, 2.0 ** 1000  # the build sends squares outside [LOW, HIGH] to the host
INT_MAX = 2 ** 31 - 1
CAND_CAP = 65536                      # kCandCap (csrc/merge.hip): more tied pairs than this and the host rescans

SCALE = {"scale-400": -400, "scale-40": -40, "scale20": 20, "scale400": 400, "cut_low": -450, "cut_high": 495,
         "under": -540, "sub": -1030, "over": 507,
         "scale17": 17}  # (the solves only: an enlarged plane whose 522 x 16 blocks all pass n * max d < INT_MAX)
MAPPED = ("neg", "shift40", "shift52", "scale-400", "scale-40", "scale20", "scale400", "cut_low", "cut_high", "under",
          "sub", "over", "mixed")                                # the generator's cities through a map
BUILT = ("midpoint", "few_bits", "special")
FAMILIES = MAPPED + BUILT
# finite, in-range squares with all 53 bits in play: where pow(dx, 2) can differ from dx*dx
GENERIC = ("neg", "scale-400", "scale-40", "scale20", "scale400", "cut_low", "cut_high", "mixed")
SIZES = (2, 12, 20)   # 1, 66 and 190 pairs: one lane, just past one wave, three passes
POOL = 256            # generator blocks the three of a comparison are picked from


def c_pow2(v):
    """The C library's pow(v, 2) (math.pow raises where C returns inf)."""
    try:
        return math.pow(v, 2)
    except OverflowError:
        return math.inf


def map_xy(name, x, y, variant=0, seed=0):
    """One block's coordinates through the family's map -> (x', y')."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if name == "neg":
        return (x - 500.0, y - 500.0) if variant % 2 == 0 else (-x, -y)
    if name == "shift40":
        return x + 2.0 ** 40, y + 2.0 ** 40
    if name == "shift52":
        return x + 2.0 ** 52, y + 2.0 ** 52
    if name in SCALE:
        return np.ldexp(x, SCALE[name]), np.ldexp(y, SCALE[name])
    if name == "mixed":
        rng = np.random.default_rng(77000 + seed)
        return (np.ldexp(x, rng.integers(-300, 301, size=x.shape)),
                np.ldexp(y, rng.integers(-300, 301, size=y.shape)))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def generated(n, B):
    """(B, n) CITY_DTYPE array of the generator's cities (./tsp n B 1000 1000)."""
    s = Shard(n, B, 0, B)
    a = np.frombuffer(s.arr, dtype=tspgpu.CITY_DTYPE).reshape(B, n).copy()
    a.setflags(write=False)
    return a


def pair_diffs(cs):
    """dx and dy of every pair i < j of every block, as the build forms them -> (2, B, pairs)."""
    n = cs.shape[1]
    i, j = np.triu_indices(n, 1)
    return np.stack([cs["x"][:, i] - cs["x"][:, j], cs["y"][:, i] - cs["y"][:, j]])


def pow_differs(d):
    """Where the C library's pow(d, 2) is another double than d*d (NaNs never count)."""
    with np.errstate(all="ignore"):
        sq = d * d
    flat = [c_pow2(v) != p and not (p != p) for v, p in zip(d.ravel().tolist(), sq.ravel().tolist())]
    return np.array(flat, dtype=bool).reshape(d.shape)


def _mapped(name, src, variants, seeds):
    out = src.copy()
    for b in range(len(src)):
        out["x"][b], out["y"][b] = map_xy(name, src["x"][b], src["y"][b], variants[b], seeds[b])
    return out


@functools.lru_cache(maxsize=None)
def _scores(name, n, variant):
    """pow(dx, 2) != dx*dx squares of every pool block under the family's map."""
    pool = generated(n, POOL)
    cs = _mapped(name, pool, [variant] * POOL, list(range(POOL)))
    return pow_differs(pair_diffs(cs)).sum(axis=(0, 2))


@functools.lru_cache(maxsize=None)
def picked(name, n, B=3):
    """Pool indices of a comparison's blocks: position k takes the unused pool
    block with the most squares on which pow and the product differ under
    the map position k gets (lowest index first among equals), so the bit
    comparison sees the fix-ups work."""
    used = []
    for k in range(B):
        sc = _scores(name, n, k % 2 if name == "neg" else 0).copy()
        sc[used] = -1
        used.append(int(np.argmax(sc)))
    return tuple(used)


def _midpoint(n, B):
    rng = np.random.default_rng(5300 + n)
    cs = np.zeros((B, n), dtype=tspgpu.CITY_DTYPE)
    cs["x"] = 2.0 * rng.integers(47453133, 67108864, size=(B, n)) + 1.0
    cs["y"] = rng.integers(0, 4000, size=(B, n)) / 4.0
    cs["x"][:, 0] = 0.0
    cs["y"][:, 0] = 0.0
    return cs


def _few_bits(n, B):
    rng = np.random.default_rng(5400 + n)
    cs = np.zeros((B, n), dtype=tspgpu.CITY_DTYPE)
    cs["x"] = rng.integers(-2048, 2049, size=(B, n)) / 4.0
    cs["y"] = rng.integers(-2048, 2049, size=(B, n)) / 4.0
    return cs


SPECIALS = (math.inf, -math.inf, math.nan, -0.0)


def _special(n, B):
    cs = generated(n, B).copy()
    for b in range(0, B, 3):
        for i in range(min(n, 4)):
            cs["x" if (i + b // 3) % 2 == 0 else "y"][b, i] = SPECIALS[(i + b // 3) % 4]
    return cs


def cities(name, n, B=3, pick=True):
    """(B, n) CITY_DTYPE array of the family.  pick: a mapped family's blocks
    are the picked pool blocks (the matrix comparisons); else the first B
    blocks of ./tsp n B 1000 1000 (the solves)."""
    if name in BUILT:
        cs = {"midpoint": _midpoint, "few_bits": _few_bits, "special": _special}[name](n, B)
        if name != "special":
            cs["id"] = np.arange(B * n).reshape(B, n)
        return cs
    if pick:
        idx = picked(name, n, B)
        src = generated(n, POOL)[list(idx)]
    else:
        idx = tuple(range(B))
        src = generated(n, B)
    cs = _mapped(name, src, list(range(B)), list(idx))
    if name == "neg":
        cs["x"][0, 0] = -0.0
    return cs


def block_lists(cs):
    """(B, n) CITY_DTYPE -> lists of (id, x, y), the form K3's Python front takes."""
    return [[(int(c["id"]), float(c["x"]), float(c["y"])) for c in blk] for blk in cs]


def squares_off_range(cs):
    """Squares of a batch the test itself finds outside [LOW, HIGH] or not finite (zero operands aside)."""
    d = pair_diffs(cs)
    with np.errstate(all="ignore"):
        sq = d * d
    return int((~((sq >= LOW) & (sq <= HIGH)) & ~(d == 0)).sum())


# ---- K3 ------------------------------------------------------------------------------------------

K3_FAMILIES = ("neg", "shift40", "shift52", "scale-400", "scale-40", "scale20")


def map_path(name, path, k=0):
    """A path of (id, x, y) through a family's map (block position k); a closing copy stays a copy."""
    closed = len(path) > 2 and path[0][0] == path[-1][0]
    body = path[:-1] if closed else path
    x, y = map_xy(name, [c[1] for c in body], [c[2] for c in body], variant=k, seed=k)
    if name == "neg" and k == 0:
        x = x.copy()
        x[0] = -0.0
    out = [(c[0], float(a), float(b)) for c, a, b in zip(body, x, y)]
    return out + [out[0]] if closed else out


def _clustered(path):
    """The outlier case's ordinary cities: snapped to a 3 x 3 grid 334 apart,
    each keeping an offset of its own below 2^-10.  Swap costs between
    clusters that would tie exactly now differ by up to a few thousandths."""
    closed = len(path) > 2 and path[0][0] == path[-1][0]
    body = path[:-1] if closed else path
    out = [(c[0], math.floor(c[1] / 334.0) * 334.0 + math.ldexp(c[1] % 1.0, -10),
            math.floor(c[2] / 334.0) * 334.0 + math.ldexp(c[2] % 1.0, -10)) for c in body]
    return out + [out[0]] if closed else out


def growing_fold(name):
    """test_merge_gpu.test_merge_matches_host's inputs (random paths, 40 blocks
    of 2..16 cities) through a K3 family, or "outlier": clustered ordinary
    cities (_clustered) and one 10^8 away, so that the candidate window,
    eps2 ~ 0.01, holds distinct near-ties -> (path, cost, [(block path, cost)] * 40)."""
    from test_merge_gpu import _random_path

    rng = np.random.default_rng(9100 + (["outlier"] + list(K3_FAMILIES)).index(name))
    fam = (lambda p, k: _clustered(p)) if name == "outlier" else (lambda p, k: map_path(name, p, k))
    acc, acc_c = _random_path(rng, 9, 0, "random")
    acc = fam(acc, 0)
    if name == "outlier":
        far = (acc[3][0], acc[3][1] + 1e8, acc[3][2])
        acc = acc[:3] + [far] + acc[4:]
    blocks = []
    for step in range(40):
        p2, c2 = _random_path(rng, int(rng.integers(2, 17)), 1000 * (step + 1), "random")
        p2 = fam(p2, step + 1)
        if len(p2) == 3:  # the n = 2 quirk: a 2-city "tour" without the closing city
            p2 = p2[1:]
        blocks.append((p2, c2))
    return acc, acc_c, blocks


def candidate_window(cs):
    """eps2 of a merge over the cities cs (csrc/merge.hip, paths_facts.h):
    2 * 2^-36 * 4 * Dmax, Dmax the padded diagonal of the bounding box."""
    xs, ys = [c[1] for c in cs], [c[2] for c in cs]
    dx, dy = max(xs) - min(xs), max(ys) - min(ys)
    dmax = math.sqrt(dx * dx + dy * dy) * (1.0 + 1e-9) + 1e-300
    return 2.0 * math.ldexp(4.0 * dmax, -36)


def glibc_swap(p1, p2, i, j):
    """Pair (i, j)'s exact swap cost: the C library's pow and sqrt, the reference's order of operations."""
    def d(a, b):
        return math.sqrt(math.pow(a[1] - b[1], 2) + math.pow(a[2] - b[2], 2))

    A, B, C, D = p1[i], p1[(i + 1) % len(p1)], p2[j], p2[(j + 1) % len(p2)]
    return ((d(A, D) + d(B, C)) - d(A, B)) - d(C, D)


def near_ties(p1, p2):
    """(pairs within the candidate window of the minimum swap cost (products
    for squares, as the device forms them), distinct exact values among them)."""
    sc = swap_costs(p1, p2)
    idx = np.argwhere(sc <= sc.min() + candidate_window(p1 + p2))
    return len(idx), len({glibc_swap(p1, p2, int(i), int(j)) for i, j in idx})


P_PT, Q_PT = (125.5, -300.25), (-1041.75, 77.0)


def overflow_merge(points):
    """A 5200-city running path and a 16-city block on two points (or one),
    distinct ids: more than CAND_CAP pairs tie at the minimum swap cost, and
    the first of them in row-major order is not pair (0, 0) on two points."""
    q = Q_PT if points == 2 else P_PT
    body1 = [(i, *P_PT) for i in range(5200)]
    body2 = [(10 ** 6 + j, *(q if j < 4 else P_PT)) for j in range(16)]
    return body1 + [body1[0]], 321.5, body2 + [body2[0]], 12.25


def exact_tied_pairs(p1, p2):
    """(pairs whose EXACT swap cost equals the minimum, the minimum, its first
    pair in row-major order), the distances being the host library's (glibc
    pow and sqrt) between the distinct points, the sums in the reference's
    order ((d(A,D) + d(B,C)) - d(A,B)) - d(C,D)."""
    pts = sorted({(c[1], c[2]) for c in p1 + p2})
    lab = {p: k for k, p in enumerate(pts)}
    d = tspgpu.distance_matrix([[(k, px, py) for k, (px, py) in enumerate(pts)] + ([(9, 0.0, 0.0)] if len(pts) < 2
                                                                                  else [])])[0]
    a = np.array([lab[(c[1], c[2])] for c in p1])
    c = np.array([lab[(c[1], c[2])] for c in p2])
    b, dd = np.roll(a, -1), np.roll(c, -1)
    A, B, C, D = a[:, None], b[:, None], c[None, :], dd[None, :]
    sc = ((d[A, D] + d[B, C]) - d[A, B]) - d[C, D]
    m = sc.min()
    return int((sc == m).sum()), float(m), tuple(int(v) for v in np.argwhere(sc == m)[0])


FOLD_OVERFLOW_B = 914


def overflow_fold_blocks(B=FOLD_OVERFLOW_B):
    """B coincident 8-city blocks: at P = 1 merge k folds a block tour of 9
    cities into a path of 8k + 1, every pair tied at 0."""
    return [[(b * 8 + i, *P_PT) for i in range(8)] for b in range(B)]


def fold_overflow_merges(B=FOLD_OVERFLOW_B):
    """Merges of that fold whose L1 * L2 pairs (all tied) exceed CAND_CAP."""
    return [k for k in range(1, B) if (8 * k + 1) * 9 > CAND_CAP]


def family_fold_blocks(kind, n, B, P, name):
    """test_persistent_fold_matches_host's blocks through a family (block b in position b)."""
    from test_pipeline_gpu import make_blocks

    return [map_path(name, blk, b) for b, blk in enumerate(make_blocks(kind, n, B, n * 1000 + B + P))]


def swap_costs(p1, p2):
    """Every pair's swap cost with products for squares (a few ulp from the exact one) -> (L1, L2)."""
    a = np.array([(c[1], c[2]) for c in p1])
    c = np.array([(c[1], c[2]) for c in p2])
    b, d = np.roll(a, -1, axis=0), np.roll(c, -1, axis=0)

    def dist(u, v):
        dx, dy = u[..., 0] - v[..., 0], u[..., 1] - v[..., 1]
        return np.sqrt(dx * dx + dy * dy)

    A, B, C, D = a[:, None, :], b[:, None, :], c[None, :, :], d[None, :, :]
    return ((dist(A, D) + dist(B, C)) - dist(A, B)) - dist(C, D)


def domain_facts(cs):
    """K3's domain over a set of (id, x, y): (all finite, smallest non-zero
    coordinate-difference square, largest).  Squares are monotone in |dx|, so
    the extremes come from neighbouring and from outermost sorted values."""
    xy = np.array([(c[1], c[2]) for c in cs], dtype=np.float64)
    lo, hi = math.inf, 0.0
    for col in (0, 1):
        u = np.unique(xy[:, col])
        if len(u) > 1:
            gap, span = float(np.diff(u).min()), float(u[-1] - u[0])
            lo, hi = min(lo, gap * gap), max(hi, span * span)
    return bool(np.isfinite(xy).all()), lo, hi


def replay_min_swaps(sols, P):
    """Needed for scale20 alone: under the other families twice the bounding
    box's diagonal is below INT_MAX, which bounds every swap cost already;
    at 2^20 it is not, so the merges themselves are looked at.

    The reference's schedule (distribution counts, every rank's left fold,
    the receives with their stale lists) over tsphost_merge -> the minimum
    swap cost (products for squares) of every merge, in schedule order."""
    B = len(sols)
    cnt = [0] * P
    for b in range(1, B + 1):
        cnt[b % P] += 1
    mins, rank, rcost, nxt = [], [], [], 0

    def merge(p1, c1, p2, c2):
        mins.append(float(swap_costs(p1, p2).min()))
        from test_merge_gpu import host_merge

        out, cost = host_merge(p1, c1, p2, c2)
        assert out is not None
        return out, cost

    for r in range(P):
        path, cost = sols[nxt]
        nxt += 1
        for _ in range(1, cnt[r]):
            path, cost = merge(path, cost, *sols[nxt])
            nxt += 1
        rank.append(list(path))
        rcost.append(cost)
    acc = [[] for _ in range(P)]

    def receive(to, frm):
        acc[to] = acc[to] + rank[frm]
        rank[to], rcost[to] = merge(rank[to], rcost[to], acc[to], rcost[frm])

    lastpower = 1 << int(math.log2(P))
    for i in range(P - lastpower):
        receive(i, i + lastpower)
    d = 0
    while (1 << d) < lastpower:
        for k in range(0, lastpower, 1 << (d + 1)):
            receive(k, k + (1 << d))
        d += 1
    return mins
