"""The coordinate families of tests/coord_families.py are what they claim, on
the CPU with numpy and the host library alone: every condition a GPU test of
test_cities_edges_gpu.py or test_merge_edges_gpu.py relies on is asserted
(and printed, run with -s) here first, so no cap or cut-off is met by accident."""
import math

import numpy as np
import pytest

import coord_families as F
import tspgpu
from test_host import _solve_all
from test_merge_gpu import host_merge

TINY = 2.0 ** -1022  # the smallest normal double


def _squares(cs):
    d = F.pair_diffs(cs)
    with np.errstate(all="ignore"):
        return d, d * d


def test_midpoint_squares_are_exact_ties():
    """Integer arithmetic: x is odd and 2^53 <= x*x < 2^54, where doubles are 2
    apart, so the odd x*x is exactly halfway between two of them; every other
    square of the block is exact."""
    ties = 0
    for n in F.SIZES:
        cs = F.cities("midpoint", n)
        for blk in cs:
            assert blk["x"][0] == 0.0 and blk["y"][0] == 0.0
            xs = [int(v) for v in blk["x"][1:]]
            for x, v in zip(xs, blk["x"][1:]):
                assert float(x) == v and x % 2 == 1 and 94906267 <= x <= 134217727
                assert 2 ** 53 <= x * x < 2 ** 54 and (x * x) % 2 == 1
                ties += 1
            for a in xs:
                for b in xs:
                    assert (a - b) ** 2 < 2 ** 53
            ys = [int(4 * v) for v in blk["y"]]
            assert all(q / 4.0 == v for q, v in zip(ys, blk["y"]))
            assert all((a - b) ** 2 < 2 ** 53 for a in ys for b in ys)
    print(f"midpoint: {ties} (0, k) x-squares, all exact ties")
    assert ties == sum(3 * (n - 1) for n in F.SIZES)


def test_cut_families_straddle_the_cutoffs():
    for name, cut in (("cut_low", F.LOW), ("cut_high", F.HIGH)):
        total = [0, 0]
        for n in F.SIZES:
            d, sq = _squares(F.cities(name, n))
            nz = sq[d != 0]
            assert np.isfinite(nz).all() and (nz > 0).all()
            below, above = int((nz < cut).sum()), int((nz > cut).sum())
            print(f"{name} n={n}: {below} squares below the cut, {above} above")
            if n >= 12:
                assert below > 0 and above > 0
            total[0] += below
            total[1] += above
        assert min(total) >= 10


def test_out_of_range_families():
    for n in F.SIZES:
        d, sq = _squares(F.cities("under", n))
        assert (sq < TINY).all() and (d != 0).all()
        cs = F.cities("sub", n)
        # (1000 * 2^-1030 is above 2^-1022: the coordinates are subnormal or in the lowest two binades;
        # every difference's square underflows to zero)
        v = np.abs(np.concatenate([cs["x"].ravel(), cs["y"].ravel()]))
        d, sq = _squares(cs)
        assert (v < 4 * TINY).all() and (v > 0).all() and (v < TINY).any() and (sq == 0).all() and (d != 0).all()
        d, sq = _squares(F.cities("over", n))
        inf, fin = int(np.isinf(sq).sum()), int(np.isfinite(sq).sum())
        print(f"over n={n}: {inf} infinite squares, {fin} finite")
        if n >= 12:
            assert inf > 0 and fin > 0
        for name in ("under", "sub"):  # the natural overflow of the fix-up list: more than a quarter flagged
            cs = F.cities(name, n)
            off, squares = F.squares_off_range(cs), 3 * n * (n - 1)
            print(f"{name} n={n}: {off} of {squares} squares outside [2^-900, 2^1000]")
            assert off > squares // 4
    for n in F.SIZES:
        c40, c52 = F.cities("shift40", n), F.cities("shift52", n)
        for f in ("x", "y"):
            assert (np.ldexp(c40[f], 12) == np.rint(np.ldexp(c40[f], 12))).all() and (c40[f] >= 2.0 ** 40).all()
            assert (c52[f] == np.rint(c52[f])).all() and (c52[f] >= 2.0 ** 52).all()
    neg = F.cities("neg", 12)
    assert (neg["x"] < 0).any() and np.signbit(neg["x"][0, 0]) and neg["x"][0, 0] == 0
    assert (neg["x"][1] < 0).all() and (neg["y"][1] < 0).all()


def test_special_mixes_every_special_value():
    seen = set()
    for n in F.SIZES:
        cs = F.cities("special", n)
        v = np.concatenate([cs["x"].ravel(), cs["y"].ravel()])
        seen |= {"+inf"} if (v == math.inf).any() else set()
        seen |= {"-inf"} if (v == -math.inf).any() else set()
        if n >= 12:
            assert np.isnan(v).any() and (np.signbit(v) & (v == 0)).any() and np.isfinite(v).sum() > v.size // 2
            assert np.isfinite(cs["x"][1:]).all() and np.isfinite(cs["y"][1:]).all()  # one special block of three
    assert seen == {"+inf", "-inf"}


def test_pow_differs_from_the_product_in_the_generic_families_only():
    total = 0
    for name in F.GENERIC:
        per = []
        for n in F.SIZES:
            cs = F.cities(name, n)
            assert np.isfinite(cs["x"]).all() and np.isfinite(cs["y"]).all()
            per.append(int(F.pow_differs(F.pair_diffs(cs)).sum()))
        print(f"{name}: pow(dx, 2) != dx*dx on {per} squares at n = {list(F.SIZES)}")
        total += sum(per)
    print(f"generic families: {total} squares with pow(dx, 2) != dx*dx")
    assert total >= 100
    for n in F.SIZES:
        assert not F.pow_differs(F.pair_diffs(F.cities("few_bits", n))).any()
        cs = F.cities("few_bits", n)
        for f in ("x", "y"):
            assert (cs[f] * 4 == np.rint(cs[f] * 4)).all() and (np.abs(cs[f]) <= 512).all()
        assert F.squares_off_range(cs) == 0


@pytest.mark.parametrize("n,B", [(12, 64), (16, 522)])
def test_solve_batches_pass_validation_where_the_gpu_test_says_so(n, B):
    """The host path solves every block of the neg, shift40, scale-40 and
    scale17 batches; under scale20 validation refuses the blocks whose n * max d
    reaches INT_MAX (the reference's sentinel), and nothing else."""
    for name in ("neg", "shift40", "scale-40", "scale17", "scale20"):
        cs = np.ascontiguousarray(F.cities(name, n, B, pick=False))
        arr = (tspgpu.City * cs.size).from_buffer_copy(cs.tobytes())
        host = tspgpu.distance_matrix_array(arr, n, B)
        status = [tspgpu.validate(host[b:b + 1]) for b in range(B)]
        refused = sum(1 for s in status if s)
        print(f"solve batch {name} n={n}: {refused} of {B} blocks refused by validation")
        if name == "scale20":
            assert all(s == (-34 if n * host[b].max() >= F.INT_MAX else 0) for b, s in enumerate(status))
            if n == 12:
                assert refused * 4 < B  # most blocks of the 2^20 plane are solved at 12 cities
        else:
            assert refused == 0


# ---- K3's constructions stay inside its domain -------------------------------------------------

def _assert_domain(cs, what):
    finite, lo, hi = F.domain_facts(cs)
    print(f"{what}: {len(cs)} cities, non-zero difference squares in [{lo:.3g}, {hi:.3g}]")
    assert finite and lo >= F.LOW and hi <= F.HIGH
    return hi


@pytest.mark.parametrize("name", ("outlier",) + F.K3_FAMILIES)
def test_growing_fold_inputs_are_in_k3s_domain(name):
    acc, acc_c, blocks = F.growing_fold(name)
    _assert_domain(acc + [c for p, _ in blocks for c in p], name)
    worst, loops, contested = -math.inf, 0, 0
    for p2, c2 in blocks:
        worst = max(worst, float(F.swap_costs(acc, p2).min()))
        if name == "outlier":
            pairs, values = F.near_ties(acc, p2)
            contested += values >= 2
        out, cost = host_merge(acc, acc_c, p2, c2)
        if out is None:
            loops += 1
            continue
        acc, acc_c = out, cost
    print(f"{name}: largest minimum swap cost {worst:.6g}, {loops} merges the reference never ends")
    assert worst < F.INT_MAX / 2 and loops < 10
    if name == "outlier":
        xs = [c[1] for c in acc]
        assert max(xs) - min(xs) >= 1e8  # Dmax ~ 1e8: eps2 = 2^-33 Dmax ~ 0.01
        eps2 = F.candidate_window(acc)
        print(f"outlier: eps2 {eps2:.6g}; {contested} of {len(blocks)} merges have at least 2 pairs within eps2 of "
              f"the minimum whose exact glibc swap costs differ")
        assert 0.011 < eps2 < 0.012 and contested >= 20


@pytest.mark.parametrize("points", (2, 1))
def test_overflow_merge_has_more_tied_pairs_than_the_candidate_buffer(points):
    p1, c1, p2, c2 = F.overflow_merge(points)
    assert len(p1) >= 4101 and len(p2) == 17
    ids = [c[0] for c in p1[:-1] + p2[:-1]]
    assert len(set(ids)) == len(ids) and len({(c[1], c[2]) for c in p1 + p2}) == points
    _assert_domain(p1 + p2, f"overflow merge on {points} point(s)")
    tied, low, first = F.exact_tied_pairs(p1, p2)
    print(f"overflow merge on {points} point(s): {tied} of {len(p1) * len(p2)} pairs tie at the minimum {low}, "
          f"first {first}")
    assert tied > F.CAND_CAP and low < F.INT_MAX
    assert first == ((0, 3) if points == 2 else (0, 0))


def test_overflow_fold_has_merges_with_more_tied_pairs_than_the_candidate_buffer():
    blocks = F.overflow_fold_blocks()
    assert len({(c[1], c[2]) for b in blocks for c in b}) == 1  # one point: every swap cost is exactly 0
    assert len({c[0] for b in blocks for c in b}) == 8 * len(blocks)
    over = F.fold_overflow_merges()
    last = (8 * (len(blocks) - 1) + 1) * 9
    print(f"overflow fold: {len(blocks)} blocks, merges {over[0]}..{over[-1]} have more than {F.CAND_CAP} tied "
          f"pairs, the last {last}")
    assert len(over) >= 3 and over[-1] == len(blocks) - 1 and last > F.CAND_CAP


@pytest.mark.parametrize("name", ("neg", "shift40"))
@pytest.mark.parametrize("kind,n,B,P", [("lattice", 6, 48, 1), ("random", 8, 300, 8)])
def test_family_folds_are_in_k3s_domain(kind, n, B, P, name):
    blocks = F.family_fold_blocks(kind, n, B, P, name)
    _assert_domain([c for b in blocks for c in b], f"{kind} {n}x{B} {name}")
    mins = F.replay_min_swaps(_solve_all(blocks), P)
    print(f"{kind} {n}x{B} P={P} {name}: {len(mins)} merges, largest minimum swap cost {max(mins):.6g}")
    assert max(mins) < F.INT_MAX / 2


@pytest.mark.parametrize("name", ("neg", "scale20"))
def test_extrema_blocks_are_in_k3s_domain(name):
    blocks = F.block_lists(F.cities(name, 8, 64, pick=False))
    _assert_domain([c for b in blocks for c in b], f"extrema {name}")
    xs = np.array([c[1] for b in blocks for c in b])
    if name == "neg":
        assert (xs < 0).any() and (xs > 0).any() and (np.signbit(xs) & (xs == 0)).any()
    sols = _solve_all(blocks)
    for P in (1, 3):
        mins = F.replay_min_swaps(sols, P)
        print(f"extrema {name} P={P}: {len(mins)} merges, largest minimum swap cost {max(mins):.6g}")
        assert max(mins) < F.INT_MAX / 2
