"""The rounding-tie family of tests/rounding_ties.py is what it claims, and K2's
host half is right on it — on the CPU, with the oracle, a plain Python DP and
the host library alone (nothing here launches a kernel).

What the GPU tests of test_rounding_ties_gpu.py rely on is asserted (and
printed, run with -s) here first: per instance |O|, whether the reverse-lex
least optimal tour is tsp()'s, and the number of backtracking steps decided
among unequal table values.  Unlike on the exact ties of test_search_host.py,
the certificate must REFUSE some of these least keys (-EAGAIN): a
tie_certify that answered 0 there would return a tour tsp() does not.
"""
import functools

import numpy as np
import pytest

import rounding_ties as R
import tspgpu
from test_search_host import records, rev_lex

EAGAIN = -11
SMALL = [s for s in R.K2_INSTANCES if s[0] <= 9]     # brute-forced
LARGE = [s for s in R.K2_INSTANCES if s[0] > 9]
K1_CHECKED = [s for n in R.K1_SIZES if n <= 13 for s in R.k1_specs(n)]


def _id(spec):
    n, kind, a, who, seed = spec
    return f"n{n}-{kind}{a}-who{who}-seed{seed}" if kind == "outlier" else f"n{n}-offset-{'sym' if a else 'asym'}-seed{seed}"


@functools.lru_cache(maxsize=None)
def dp_facts(spec):
    """(cost, tour, rounding-tie steps, least optimal tour) by the Python DP (the table itself is not kept)."""
    d = R.build(spec)
    cost, tour, G = R.held_karp(d)
    return cost, tuple(tour), R.rounding_tie_steps(d, tour, G), R.least_optimal_tour(d, G)


@functools.lru_cache(maxsize=None)
def brute(spec):
    """(optimum, O) by brute force, n <= 9."""
    opt, oset = R.optimal_set(R.build(spec))
    return opt, tuple(oset)


def certified_expected(spec):
    """The least key must be certified exactly when it is tsp()'s tour."""
    return [0, *dp_facts(spec)[3], 0] == list(R.reference(spec)[1])


def test_helpers_on_known_cases():
    """fold_is_exact is tie_certify's shortcut; scaled is exact above the
    subnormals; largest_scale is the last k that passes n * max(d) < INT_MAX."""
    ints = np.random.default_rng(1).integers(1, 6, (7, 7)).astype(np.float64)
    assert R.fold_is_exact(ints) and R.fold_is_exact(ints * 2.0 ** -30) and R.fold_is_exact(np.zeros((5, 5)))
    assert not R.fold_is_exact(R.scale_base(9, "uniform"))
    big = ints.copy()
    big[0, 1] = 2.0 ** 53                                  # integers, but 7 * max is past 2^53
    assert not R.fold_is_exact(big)
    for n in R.SCALE_SIZES:
        for kind in ("uniform", "lattice"):
            d = R.scale_base(n, kind)
            ks = []
            for knd, k, m in R.scale_cases(n):
                if knd != kind:
                    continue
                ks.append(k)
                assert (m >= 0).all() and np.isfinite(m).all() and n * m.max() < R.INT_MAX
                if k >= -400:
                    assert np.array_equal(np.ldexp(m, -k), d)  # exact
                else:
                    nz = m[d != 0]
                    assert (nz < 2.0 ** -1022).all() and (nz > 0).all()  # subnormal entries
            top = ks[-1]
            assert n * float(np.ldexp(d.max(), top + 1)) >= R.INT_MAX and top > 10
            print(f"scale n={n} {kind}: k = {ks}")


@pytest.mark.parametrize("spec", list(R.K2_INSTANCES) + K1_CHECKED, ids=_id)
def test_python_dp_equals_the_oracle(spec):
    """The plain DP (the reference's fold order, first strict minimum,
    first-equal backtracking) gives the oracle's cost bits and tour."""
    cost, tour, _, _ = dp_facts(spec)
    oc, ot = R.reference(spec)
    assert cost == oc and list(tour) == ot


@pytest.mark.parametrize("spec", SMALL, ids=_id)
def test_host_half_on_the_brute_forced_set(spec):
    """n = 8, 9 with O by brute force: the fold is not exact (the certificate's
    shortcut does not apply), several tours tie, the host rule over all of O
    gives tsp()'s tour, and the least key is certified exactly when it is that
    tour — never certified as another one — by the prefix DP and by the
    records of O alike."""
    d = R.build(spec)
    opt, oset = brute(spec)
    oc, ot = R.reference(spec)
    assert opt == oc
    assert not R.fold_is_exact(d)
    assert len(oset) > 1
    assert len({R.left_fold(d, p) for p in oset}) == 1
    recs = records(oset, opt, tspgpu.F64)
    assert tspgpu.select_tour(d, recs, opt).tolist() == ot
    least = min(oset, key=lambda p: tspgpu.tie_key([0, *p, 0]))
    assert least == min(oset, key=rev_lex) == dp_facts(spec)[3]
    w0, w1 = tspgpu.tie_key([0, *least, 0])
    same = [0, *least, 0] == ot
    rc, tour = tspgpu.tie_tour(d, w0, w1, opt)
    rc_r, tour_r = tspgpu.tie_tour_records(None, d, w0, w1, opt, recs)
    print(f"{_id(spec)}: |O| = {len(oset)}, least key is tsp()'s tour: {same}, "
          f"rounding-tie steps {dp_facts(spec)[2]}, tie_tour {rc}, tie_tour_records {rc_r}")
    if same:
        assert rc == 0 and tour.tolist() == ot
        assert rc_r == 0 and tour_r.tolist() == ot
    else:
        assert rc == EAGAIN and rc_r == EAGAIN
    # the certificate proves a tour DP-consistent: tsp()'s is the least of those, not of all of O
    if len(oset) <= 64:
        rcs = {p: tspgpu.tie_tour(d, *tspgpu.tie_key([0, *p, 0]), opt)[0] for p in oset}
        assert set(rcs.values()) <= {0, EAGAIN}
        assert [0, *min((p for p in oset if rcs[p] == 0), key=rev_lex), 0] == ot


@pytest.mark.parametrize("spec", LARGE, ids=_id)
def test_host_half_above_brute_force(spec):
    """n = 11, 13: the least optimal tour from the DP table (least_optimal_tour,
    equal to brute force at 8 and 9 above); the certificate answers 0 with
    tsp()'s tour or -EAGAIN, as that tour is or is not tsp()'s."""
    d = R.build(spec)
    oc, ot = R.reference(spec)
    least = dp_facts(spec)[3]
    assert R.left_fold(d, least) == oc and not R.fold_is_exact(d)
    w0, w1 = tspgpu.tie_key([0, *least, 0])
    rc, tour = tspgpu.tie_tour(d, w0, w1, oc)
    same = certified_expected(spec)
    print(f"{_id(spec)}: least key is tsp()'s tour: {same}, rounding-tie steps {dp_facts(spec)[2]}, tie_tour {rc}")
    assert (rc == 0 and tour.tolist() == ot) if same else rc == EAGAIN


def test_the_certificate_refuses_some_and_certifies_some():
    """On exact ties every least key certifies (test_search_host.py asserts
    certified == total).  Not here: at least 4 of the brute-forced instances
    have a least key that is not tsp()'s tour (condition on the seed list), and
    every size has both outcomes for the GPU test to meet."""
    refused = [s for s in SMALL if not certified_expected(s)]
    print(f"brute-forced: {len(refused)} of {len(SMALL)} least keys refused")
    assert len(refused) >= 4 and len(refused) < len(SMALL)
    for n in (8, 9, 11, 13):
        got = {certified_expected(s) for s in R.K2_INSTANCES if s[0] == n}
        assert got == {True, False}, n
    assert sum(1 for s in R.K2_INSTANCES if s[0] == 13) <= 8  # (the heavy ones of the GPU test)


def test_every_gpu_instance_has_a_rounding_tie_step():
    """The oracle's backtracking on every matrix the GPU tests use at n <= 13
    has a step where members with different table values reach the target.
    The one corner where that cannot happen (outlier at city 0, s = -34: all
    other edges are below half an ulp of the first) is checked to be that."""
    for spec in list(R.K2_INSTANCES) + K1_CHECKED:
        steps = dp_facts(spec)[2]
        print(f"{_id(spec)}: {steps} rounding-tie steps")
        if R.absorbs_everything(spec):
            d = R.build(spec)
            half_ulp = np.spacing(d[0, 1:].min()) / 2
            assert d[1:, 1:].max() < half_ulp and steps == 0
        else:
            assert steps >= 1, spec
    for n in R.K1_SIZES:
        mats = [R.build(s) for s in R.k1_specs(n)]
        assert len({m.tobytes() for m in mats}) == 16
        assert all(n * m.max() < R.INT_MAX for m in mats)
    for n in R.WIDE_K1_SIZES:
        mats = [R.build(s) for s in R.wide_specs(n)]
        assert len({m.tobytes() for m in mats}) == 10 and all(n * m.max() < R.INT_MAX for m in mats)
