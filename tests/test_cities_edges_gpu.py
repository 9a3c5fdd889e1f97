"""The device distance build (csrc/cities.hip, csrc/dist_exact.h) off the
generator's coordinates: the families of tests/coord_families.py (negative,
translated, rescaled, straddling the 2^-900 and 2^1000 cut-offs, subnormal,
overflowing, exact midpoints, non-finite) against the host path with glibc's
pow and sqrt (tspgpu.distance_matrix_array, Context.solve_cities).

Nothing here has a tolerance: matrices and costs are compared as uint64 bits
(where the host has a NaN the device must have one at the same place: the
header excludes only the payload), tours entry by entry, statuses with
tspgpu.validate on the host matrix.  tests/test_coord_families.py proves on
the CPU what every family is relied on for here."""
import errno

import numpy as np
import pytest

import coord_families as F
import tspgpu
from test_cities_device_gpu import _carray, _device_dist, _host_dist, _solve_device
from test_cities_ragged_gpu import device_dist as ragged_device_dist

pytestmark = pytest.mark.gpu

U64 = np.uint64
ERANGE = -errno.ERANGE
_uniform = {}  # (family, n) -> the device's (3, n, n) matrices, shared with the ragged test


def _assert_bits(got, want, what):
    nan = np.isnan(want)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.argwhere(got.view(U64)[...] != want.view(U64)[...])
    bad = [tuple(int(v) for v in p) for p in bad if not nan[tuple(p)]]
    assert not bad, f"{what}: {len(bad)} entries differ, first {bad[:4]}"


def _uniform_dist(ctx, name, n):
    """(device matrices, fix-up statistics) of the family's three n-city blocks, built once."""
    if (name, n) not in _uniform:
        got = _device_dist(ctx, F.cities(name, n))
        _uniform[name, n] = (got, ctx.cities_last_fixups())
    return _uniform[name, n]


@pytest.mark.parametrize("n", F.SIZES)
@pytest.mark.parametrize("name", F.FAMILIES)
def test_matrix_bits_and_fixup_statistics(gpu_ctx, name, n):
    """3 blocks of 2, 12 and 20 cities (1, 66 and 190 pairs).  The statistics:
    two squares per pair; at least the squares this test finds outside
    [2^-900, 2^1000] or non-finite are flagged (dx and dx*dx in numpy, not the
    rule); exact squares flag nothing (few_bits; in midpoint everything but
    the (0, k) x-squares, which are exact ties and all flagged); a second
    build pass exactly when the flagged squares outgrow the default list of a
    quarter of the squares, which under and sub do on their own."""
    cs = F.cities(name, n)
    got, (sq, flagged, passes) = _uniform_dist(gpu_ctx, name, n)
    off = F.squares_off_range(cs)
    print(f"STATS {name} n={n}: squares {sq} flagged {flagged} passes {passes} (off-range or non-finite {off})")
    _assert_bits(got, _host_dist(cs), f"{name} n={n}")
    assert sq == 3 * n * (n - 1)
    assert off <= flagged <= sq
    assert passes == (2 if flagged > sq // 4 else 1)
    if name == "few_bits":
        assert flagged == 0
    if name == "midpoint":
        assert flagged == 3 * (n - 1)
    if name in ("under", "sub"):
        assert passes == 2 and flagged == sq


CYCLE = (1, 2, 12, 13, 20)


def test_ragged_build_equals_the_uniform_builds(gpu_ctx):
    """One packed call over every family, sizes cycling through 1, 2, 12, 13
    and 20: each block's bits are those of its uniform three-block build."""
    blocks, want = [], []
    for fi, name in enumerate(F.FAMILIES):
        for b in range(3):
            n = CYCLE[(3 * fi + b) % len(CYCLE)]
            blocks.append(F.cities(name, n)[b].copy())
            want.append((name, n, b))
    uniform = [_uniform_dist(gpu_ctx, name, n)[0][b] for name, n, b in want]
    got = ragged_device_dist(gpu_ctx, blocks)
    sq, flagged, passes = gpu_ctx.cities_last_fixups()
    print(f"STATS ragged: squares {sq} flagged {flagged} passes {passes}")
    assert sq == sum(len(b) * (len(b) - 1) for b in blocks)
    assert passes == (2 if flagged > sq // 4 else 1)
    assert sum(F.squares_off_range(blk[None, :]) for blk in blocks) <= flagged <= sq
    for (name, n, b), g, u, blk in zip(want, got, uniform, blocks):
        _assert_bits(g, u, f"ragged {name} n={n} block {b} against the uniform build")
        _assert_bits(g, tspgpu.distance_matrix_array(_carray(blk), n, 1)[0], f"ragged {name} n={n} block {b}")


def _assert_solves(ctx, cs):
    """solve_cities_device against tspgpu.validate and Context.solve_cities on
    the same cities, block by block -> the host's statuses."""
    B, n = cs.shape
    host = _host_dist(cs)
    want_status = [tspgpu.validate(host[b:b + 1]) for b in range(B)]
    good = [b for b in range(B) if not want_status[b]]
    cost, tour, status = _solve_device(ctx, cs)
    assert status.tolist() == want_status
    for b in range(B):
        if want_status[b]:
            assert np.isnan(cost[b]) and (tour[b] == -1).all(), (b, cost[b], tour[b].tolist())
    if good:
        want_cost, want_tour = ctx.solve_cities((_carray(cs[good]), n, len(good)))
        assert np.array_equal(cost[good].view(U64), want_cost.view(U64))
        assert np.array_equal(tour[good], want_tour)
    return want_status


@pytest.mark.parametrize("n", (12, 16))
@pytest.mark.parametrize("name", ("neg", "shift40", "scale-40", "scale17", "scale20"))
def test_solves_equal_the_host_path(gpu_ctx, name, n):
    """64 blocks of 12 cities, 522 of 16 (a full wave of blocks: K1 variant 6).
    Every status is 0, except under scale20, where a block whose n * max d
    reaches INT_MAX is refused by validation on both paths (-ERANGE, NaN, a
    row of -1): none of 64 at 12 cities, all 522 at 16, whose tiles are 500
    wide.  scale17 is the enlarged plane that variant 6 does solve."""
    B = 522 if n == 16 else 64
    cs = F.cities(name, n, B, pick=False)
    status = _assert_solves(gpu_ctx, cs)
    variant = gpu_ctx.last_variant()
    print(f"STATS solve {name} n={n}: {B - sum(1 for s in status if s)} of {B} blocks solved, variant {variant}")
    if name == "scale20":
        assert set(status) <= {0, ERANGE}
    else:
        assert not any(status)
        if n == 16:
            assert variant == 6


@pytest.mark.parametrize("n", (12, 16))
@pytest.mark.parametrize("name", ("over", "special"))
def test_bad_blocks_get_the_hosts_status(gpu_ctx, name, n):
    """Infinite squares (over) and non-finite coordinates (special): every
    block gets the status tspgpu.validate gives its host matrix, a bad one a
    NaN cost and a tour row of -1, a good one the host's bits."""
    B = 522 if n == 16 else 64
    status = _assert_solves(gpu_ctx, F.cities(name, n, B, pick=False))
    bad = sum(1 for s in status if s)
    print(f"STATS solve {name} n={n}: {bad} of {B} blocks refused")
    assert bad == (B if name == "over" else (B + 2) // 3)
