"""K2, K1, the ragged batch and K1-wide on tours that tie only after rounding
(tests/rounding_ties.py; what the family is, and K2's host half on it, is
proven on the CPU in test_rounding_ties.py), and all three solvers on ordinary
instances scaled by powers of two.  Cost bits and tours only: nothing here has
a tolerance.

K2 runs at n = 8, 9, 11 and 13 and NEVER LARGER.  On this family every tour
lies within the pruning margin of the optimum, so no bound prunes and the
search is the full (n-1)! enumeration: 4.8e8 leaves at 13 cities
(milliseconds), 1.3e12 at 16.  Do not raise n "to see".

How a K2 solve can end (read from its statistics), and where it was met on an
MI355X — the coverage test asserts every ending over the instance list:

ending (statistics)              default settings, instances per size          with a knob
-------------------------------  --------------------------------------------  ------------------------------------
device tie rule certified        n = 8: 2 of 9, 9: 2 of 9, 11: 6 of 8,         SEARCH_RECORD_CAP=2 (the certificate
(tie 1)                          13: 4 of 8                                    with every prefix DP): exactly the
                                                                               instances whose least key is tsp()'s
certificate refused, the         n = 8: 7, 9: 7, 11: 1 (s = -30, who 0),       SEARCH_TIE=0: every instance whose
records decide (tie 0,           13: 3 (s = -32 who 0, s = -28 who 6,          records fit (all at 8 and 9)
phases 1, fallback 0)            s = -30 who 12).  At 8 and 9 this includes
                                 certifiable keys: while 513 .. 65536 records
                                 fit the buffer the certificate runs without
                                 its prefix DP and the records answer
second phase (phases 2)          n = 11, s = -34, who 5, seed 0: refused,      SEARCH_RECORD_CAP=2 on every refused
                                 1.4e6 optimal tours of 3.6e6                  instance, with SEARCH_TIE=0 on all
K1-wide fallback (fallback 1)    n = 13, s = -34, who 6, seed 2: refused,      SEARCH_TIE=0: also s = -34 who 6
                                 1.8e8 records (more than a second phase       seed 1 and the symmetric offset
                                 may hold)                                     matrix (1.7e8 and 9.4e7 records)

No ending needs a knob.  The heaviest solve (13 cities, 1.8e8 records) takes 0.48 s of kernel time.
"""
import errno

import numpy as np
import pytest

import oracle_py as O
import rounding_ties as R
import search_dist
import tspgpu
from test_rounding_ties import _id, brute, certified_expected, dp_facts

pytestmark = pytest.mark.gpu

F64 = np.float64


def _bits(c):
    """IEEE bits: an int for a scalar, a uint64 array for an array."""
    a = np.asarray(c, dtype=F64).view(np.uint64)
    return int(a) if a.ndim == 0 else a


# ---- K2 --------------------------------------------------------------------------------------------

def k2_settings(n):
    """(name, knobs, exhaustive) of every way an instance is searched."""
    out = [("default", {}, False), ("tie0", {"SEARCH_TIE": 0}, False), ("cap2", {"SEARCH_RECORD_CAP": 2}, False),
           ("cap2_tie0", {"SEARCH_RECORD_CAP": 2, "SEARCH_TIE": 0}, False), ("enum", {}, True)]
    if n <= 11:
        out += [("enum_rounds", {"ENUM_KERNEL": 0}, True), ("kernel1", {"SEARCH_KERNEL": 1}, False),
                ("kernel2", {"SEARCH_KERNEL": 2}, False)]
    return out + [(f"tail{t}", {"SEARCH_TAIL": t}, False) for t in (0, 5, 6)]


def ending(st):
    if st["fallback"]:
        return "fallback"
    if st["phases"] == 2:
        return "phases2"
    return "tie" if st["tie"] else "records"


_RUNS = {}


def k2_runs(ctx, knobs, spec):
    """Every setting's (name, cost, tour, stats) of an instance, searched once per session."""
    if spec not in _RUNS:
        d, out = R.build(spec), []
        for name, kn, exhaustive in k2_settings(spec[0]):
            knobs.clear()
            for k, v in kn.items():
                knobs.set(k, v)
            cost, tour, st = tspgpu.search_solve(ctx, d, exhaustive=exhaustive)
            out.append((name, cost, tour.tolist(), st))
        knobs.clear()
        _RUNS[spec] = out
    return _RUNS[spec]


@pytest.mark.parametrize("spec", R.K2_INSTANCES, ids=_id)
def test_k2_every_setting_gives_the_oracle_answer(gpu_ctx, knobs, spec):
    """search_solve with the default settings, without the device tie rule,
    with a 2-record buffer (with and without it), by exhaustive enumeration
    (enum.hip; the round kernels at n <= 11), with each round kernel (n <= 11)
    and with the DFS rounds and both register tails: the oracle's cost bits
    and tour.  The device tie rule's answer is used only where the host test
    says the least key is tsp()'s tour; with the 2-record buffer (the full
    certificate) exactly there.  At 8 and 9 cities, whenever the records were
    read in one phase, they hold all of O (brute force) and nothing else at
    that cost."""
    oc, ot = R.reference(spec)
    expected = certified_expected(spec)
    n_opt = len(brute(spec)[1]) if spec[0] <= 9 else None
    for name, cost, tour, st in k2_runs(gpu_ctx, knobs, spec):
        print(f"{_id(spec)} {name}: {ending(st)}, records {st['records']}, optimal_tours {st['optimal_tours']}, "
              f"tie_checked {st['tie_checked']}, nodes {st['nodes']}, kernel {st['kernel_ms']:.2f} ms")
        assert (_bits(cost), tour) == (_bits(oc), ot), (name, st)
        assert st["tie_checked"] != -1, (name, st)
        if st["tie"]:
            assert expected and not st["fallback"] and st["phases"] == 1, (name, st)
        if "tie0" in name:
            assert st["tie"] == 0, (name, st)
        if name == "cap2":  # (the buffer overflowed: the certificate with every prefix DP)
            assert st["tie"] == int(expected), (name, st)
        if n_opt is not None and st["phases"] == 1 and not st["fallback"]:
            if st["tie"] and st["tie_checked"] == 0:
                assert st["optimal_tours"] == 0, (name, st)  # (certified without reading the records: not counted)
            else:
                assert st["optimal_tours"] == n_opt, (name, st)
        if n_opt is not None and name == "tie0":  # (40320 tours at most: the records always fit)
            assert st["phases"] == 1 and not st["fallback"] and st["optimal_tours"] == n_opt, st


def test_k2_every_ending_is_met(gpu_ctx, knobs):
    """Over the whole instance list each ending occurs: the device tie rule
    certified; the certificate refused and the records decided in one phase;
    a second phase; the K1-wide fallback.  (The table in the module docstring.)"""
    met = {}
    for spec in R.K2_INSTANCES:
        for name, _, _, st in k2_runs(gpu_ctx, knobs, spec):
            met.setdefault(ending(st), {}).setdefault((spec[0], name), []).append(_id(spec))
    for e in ("tie", "records", "phases2", "fallback"):
        for (n, name), ids in sorted(met.get(e, {}).items()):
            print(f"{e}: n = {n} {name}: {len(ids)} instances")
    assert set(met) == {"tie", "records", "phases2", "fallback"}, sorted(met)
    # without a knob: the default settings alone reach all four, and refuse where the host test says so
    default = {s: ending(next(r for r in k2_runs(gpu_ctx, knobs, s) if r[0] == "default")[3]) for s in R.K2_INSTANCES}
    assert set(default.values()) == {"tie", "records", "phases2", "fallback"}, default
    assert all(e != "tie" for s, e in default.items() if not certified_expected(s))


@pytest.mark.parametrize("spec", R.K2_INSTANCES, ids=_id)
def test_k2_sharded_driver_and_three_shards(gpu_ctx, knobs, spec):
    """search_dist.solve_sharded (one rank), chained and step by step: the
    oracle's answer, the winning key certified exactly where the host test
    predicts and the records asked otherwise.  Then three shards on one GPU
    (as test_chain_tie_slot_abi): the MIN of their keys at the optimum IS the
    host test's least key, tspgpu_tie_tour certifies or refuses it as
    predicted, and the union of the shards' records gives tsp()'s tour."""
    d = R.build(spec)
    oc, ot = R.reference(spec)
    expected = certified_expected(spec)
    for chain in (True, False):
        knobs.clear()
        if not chain:
            knobs.set("SEARCH_CHAIN", 0)
        cost, tour, st = search_dist.solve_sharded(gpu_ctx, d)
        print(f"{_id(spec)} sharded chain={int(chain)}: tie {st['tie']} phases {st['phases']} fallback "
              f"{st['fallback']} chained {st['chained']}")
        assert (_bits(cost), tour.tolist()) == (_bits(oc), ot), (chain, st)
        assert st["tie"] == int(expected) and st["record_gather"] == 1 - st["tie"], (chain, st)
        if not chain:
            assert st["chained"] == 0, st
    knobs.clear()
    ub, _ = tspgpu.heuristic_tour(d)
    shards = [tspgpu.Search(gpu_ctx, d, shard=s, nshards=3) for s in range(3)]
    try:
        for S in shards:
            S.set_bound(ub)
            if not S.chain():
                S.run_all()
        opt = min(S.counters()[0] for S in shards)
        assert opt == tspgpu.cost_bits(oc, tspgpu.F64)
        slots = [S.tie_slot(opt) for S in shards]
        assert not any(ovf for _, _, _, ovf in slots) and any(f for f, _, _, _ in slots), slots
        w0 = min(w for f, w, _, _ in slots if f)
        assert w0 == tspgpu.tie_key([0, *dp_facts(spec)[3], 0])[0]
        rc, tour = tspgpu.tie_tour(d, w0, 0, oc)
        assert (rc == 0 and tour.tolist() == ot) if expected else rc == -errno.EAGAIN
        rc_g, tour_g = tspgpu.tie_tour_gpu(gpu_ctx, d, w0, 0, oc)  # (the prefix DPs on the GPU above 12 cities)
        assert (rc_g == 0 and tour_g.tolist() == ot) if expected else rc_g == -errno.EAGAIN
        try:
            recs = [r for S in shards for r in S.records(opt)]
        except tspgpu.TspGpuError as e:
            assert e.code == -errno.EOVERFLOW and spec[0] > 9  # (a shard lost records: only above 9 cities)
            recs = None
        if recs is not None:
            assert tspgpu.select_tour(d, recs, oc).tolist() == ot
            if spec[0] <= 9:
                assert len(recs) == len(brute(spec)[1])
            rc_r, tour_r = tspgpu.tie_tour_records(gpu_ctx, d, w0, 0, oc, recs)
            assert (rc_r == 0 and tour_r.tolist() == ot) if expected else rc_r == -errno.EAGAIN
    finally:
        for S in shards:
            S.close()


# ---- K1, the ragged batch, K1-wide -----------------------------------------------------------------

_REF = {}


def k1_reference(n):
    """(16 distinct matrices, oracle cost bits, oracle tours) of a size, solved once."""
    if n not in _REF:
        specs = R.k1_specs(n)
        d = np.ascontiguousarray(np.array([R.build(s) for s in specs]), dtype=F64)
        res = [R.reference(s) for s in specs]
        bits = np.array([r[0] for r in res], dtype=F64).view(np.uint64).copy()
        tours = np.array([r[1] for r in res], dtype=np.int32)
        for a in (d, bits, tours):
            a.setflags(write=False)
        _REF[n] = (d, bits, tours)
    return _REF[n]


def _run_twice_and_compare(ctx, batch, src, bits, tours):
    first = ctx.solve_blocks(batch)
    second = ctx.solve_blocks(batch)
    assert np.array_equal(_bits(first[0]), _bits(second[0])) and np.array_equal(first[1], second[1])
    T = tours.shape[1]
    bad = np.flatnonzero((_bits(first[0]) != bits[src]) | (first[1][:, :T] != tours[src]).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {batch.shape[0]} blocks differ from the oracle, first {bad[:5].tolist()}"


@pytest.mark.parametrize("n", R.K1_SIZES)
def test_k1_batches_match_the_oracle_bit_for_bit(gpu_ctx, knobs, n):
    """The size's 16 family matrices tiled into 2 x CUs + 1 blocks, at the
    product's occupancy and with one workgroup per CU (every persistent loop
    runs at least twice): two runs identical, every row the oracle's cost bits
    and tour — the `c == target` ballots of the backtracking decide among
    rounding ties on every one of them (n <= 13: asserted on the CPU)."""
    d, bits, tours = k1_reference(n)
    cu = gpu_ctx.device_info()[0]
    B = 2 * cu + 1
    src = np.random.default_rng(n).integers(0, 16, B)
    src[:16] = np.arange(16)  # (every distinct matrix is in the batch)
    batch = np.ascontiguousarray(d[src])
    _run_twice_and_compare(gpu_ctx, batch, src, bits, tours)
    try:
        knobs.set("WG_PER_CU", 1)
        ctx = tspgpu.Context(device=0)
    finally:
        knobs.clear()
    try:
        _run_twice_and_compare(ctx, batch, src, bits, tours)
    finally:
        ctx.close()


def test_ragged_batch_of_every_size(gpu_ctx):
    """The same 7 x 16 matrices, sizes mixed in one Context.solve_ragged call:
    status 0 everywhere, the oracle's cost bits and tours, twice the same."""
    blocks = [(n, b) for n in R.K1_SIZES for b in range(16)]
    order = np.random.default_rng(16).permutation(len(blocks))
    mats = [k1_reference(blocks[i][0])[0][blocks[i][1]] for i in order]
    first = gpu_ctx.solve_ragged(mats)
    second = gpu_ctx.solve_ragged(mats)
    cost, tour, status = first
    assert np.array_equal(_bits(cost), _bits(second[0])) and np.array_equal(tour, second[1])
    assert np.array_equal(status, second[2])
    assert not status.any(), status.tolist()
    for row, i in enumerate(order):
        n, b = blocks[i]
        _, bits, tours = k1_reference(n)
        assert _bits(cost[row]) == bits[b], (n, b)
        assert tour[row, :n + 1].tolist() == tours[b].tolist() and (tour[row, n + 1:] == -1).all(), (n, b)


@pytest.mark.parametrize("n", R.WIDE_ORACLE_SIZES)
def test_k1_wide_matches_the_oracle(gpu_ctx, n):
    """Context.solve_instance on the size's 16 family matrices: the oracle's bits and tour."""
    d, bits, tours = k1_reference(n)
    for b in range(16):
        cost, tour, _ = gpu_ctx.solve_instance(d[b])
        assert _bits(cost) == bits[b] and tour.tolist() == tours[b].tolist(), (n, R.k1_specs(n)[b])
        assert gpu_ctx.wide_last_dtype() == tspgpu.F64


@pytest.mark.parametrize("n", R.WIDE_K1_SIZES)
def test_k1_wide_matches_k1_at_18_and_20(gpu_ctx, n):
    """Above the oracle's reach K1-wide (its pull and its push layers) and K1
    solve the same 10 family matrices: identical cost bits and tours."""
    specs = R.wide_specs(n)
    d = np.ascontiguousarray(np.array([R.build(s) for s in specs]), dtype=F64)
    c1, t1 = gpu_ctx.solve_blocks(d)
    for b, spec in enumerate(specs):
        cost, tour, _ = gpu_ctx.solve_instance(d[b])
        assert _bits(cost) == _bits(c1[b]) and tour.tolist() == t1[b].tolist(), spec
        assert sorted(tour[:-1].tolist()) == list(range(n)) and tour[0] == tour[-1] == 0


# ---- power-of-two scale ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SCALE_SIZES)
def test_power_of_two_scale(gpu_ctx, knobs, n):
    """A uniform and a 4 x 4-lattice instance times 2^k, k = -1040 (subnormal
    entries), -400, -60, -20, 10 and the largest that keeps n * max(d) below
    INT_MAX: K1, K1-wide and K2 (default; the tree bound at every level with
    and without the Lagrangian weights) each return the oracle's answer on
    that same scaled matrix.  K2's bound tables carry absolute constants (a
    2^-20 grid, + 1.0 in the margins), so at small scales its bounds lose
    their force and the node count grows to the full enumeration (printed,
    not asserted: node counts depend on incumbent timing).
    n stays <= 13 for that reason."""
    cases = R.scale_cases(n)
    ref = [O.solve_block(m) for _, _, m in cases]
    batch = np.ascontiguousarray(np.array([m for _, _, m in cases]), dtype=F64)
    c1, t1 = gpu_ctx.solve_blocks(batch)
    for i, ((kind, k, m), (oc, ot)) in enumerate(zip(cases, ref)):
        assert _bits(c1[i]) == _bits(oc) and t1[i].tolist() == ot, ("K1", kind, k)
        cw, tw, _ = gpu_ctx.solve_instance(m)
        assert _bits(cw) == _bits(oc) and tw.tolist() == ot, ("K1-wide", kind, k)
        nodes = []
        for kn in ({}, {"SEARCH_MST_MINREM": 0, "SEARCH_LAGRANGE": 1}, {"SEARCH_MST_MINREM": 0, "SEARCH_LAGRANGE": 0}):
            knobs.clear()
            for name, v in kn.items():
                knobs.set(name, v)
            cost, tour, st = tspgpu.search_solve(gpu_ctx, m)
            assert (_bits(cost), tour.tolist()) == (_bits(oc), ot), ("K2", kind, k, kn, st)
            nodes.append(st["nodes"])
        knobs.clear()
        print(f"scale n={n} {kind} k={k}: K2 nodes default {nodes[0]}, tree bound everywhere {nodes[1]}, "
              f"without Lagrange {nodes[2]}")
