"""The exhaustive enumeration as S shards (TSPGPU_SEARCH_EXHAUSTIVE,
tspgpu.Search(..., exhaustive=True)), the shards run one after another on one
GPU: shard s folds the prefixes p = i*S + s.  Every shard count must give the
oracle's bit-exact cost and tie-broken tour, and the shards' node counts must
sum to every partial path exactly."""
import errno
import math
import signal

import numpy as np
import pytest

import oracle_py as O
import tspgpu

pytestmark = pytest.mark.gpu


def _enum_nodes(n):
    N = n - 1
    return sum(math.factorial(N) // math.factorial(N - l) for l in range(1, N + 1))


def _cities_matrix(n, rng, lattice):
    xy = rng.integers(0, 4, size=(n, 2)).astype(np.float64) if lattice else rng.uniform(0, 1000, size=(n, 2))
    return O.distance_matrix([(i, xy[i, 0], xy[i, 1]) for i in range(n)])


def _oracle(d):
    if np.asarray(d).dtype == np.int32:
        oc, ot = O.solve_block(np.asarray(d).astype(np.int64))
        return int(oc), ot
    return O.solve_block(d)


def _open(ctx, d, S):
    """The S shards with the same host-heuristic bound."""
    ub, _ = tspgpu.heuristic_tour(d)
    shards = [tspgpu.Search(ctx, d, shard=s, nshards=S, exhaustive=True) for s in range(S)]
    for X in shards:
        X.set_bound(ub)
    assert sum(X.local_items for X in shards) == shards[0].items
    assert all(X.items == shards[0].items and X.depth == shards[0].depth for X in shards)
    for s, X in enumerate(shards):
        assert X.local_items == X.items // S + (1 if X.items % S > s else 0)
    return shards, tspgpu.cost_bits(ub, shards[0].dtype)


def _run(shards, mode):
    for X in shards:
        if mode == "run_all":
            X.run_all()
            continue
        calls = []
        done = X.chain(2, hook=lambda st, w: calls.append(1))
        if mode == "chain":
            assert done is True and calls == []  # one launch, no level: the hook is never called
        else:  # "steps": the round kernels with the bound off are no chain
            assert done is False
            X.start()
            while X.step():
                pass


def _winner(ctx, d, shards, use_records=False):
    """MIN of the incumbents, then MIN of the tie keys of the shards that hold a
    tour of that cost; the records (select_tour) when a tie table overflowed.
    -> (cost, tour, answered by the tie key)."""
    dt = shards[0].dtype
    opt = min(X.counters()[0] for X in shards)
    cost = tspgpu.bits_cost(opt, dt)
    slots = [X.tie_slot(opt) for X in shards]
    if not use_records and not any(ovf for _, _, _, ovf in slots):
        w0, w1 = min((w0, w1) for found, w0, w1, _ in slots if found)
        rc, tour = tspgpu.tie_tour_gpu(ctx, d, w0, w1, cost)
        if rc == 0:
            return cost, tour.tolist(), True
        assert rc == -errno.EAGAIN  # a valid tour the certificate cannot prove: the records decide
    recs = [r for X in shards for r in X.records(opt)]
    return cost, tspgpu.select_tour(d, recs, cost).tolist(), False


def _close(shards):
    for X in shards:
        X.close()


def _check(ctx, d, S, mode="chain"):
    shards, ub_bits = _open(ctx, d, S)
    try:
        _run(shards, mode)
        cost, tour, _ = _winner(ctx, d, shards)
        assert (cost, tour) == _oracle(d), (len(d), S, mode)
        nodes = [X.counters()[1] for X in shards]
        for X, nd in zip(shards, nodes):
            if X.local_items == 0:  # an empty shard folds nothing and keeps the bound
                assert nd == 0 and X.counters()[0] == ub_bits and X.tie_slot(ub_bits)[0] is False
        return nodes, shards[0].depth
    finally:
        _close(shards)


@pytest.mark.parametrize("n,S", [(7, 3), (8, 3), (8, 8)])
def test_fewer_prefixes_than_shards(gpu_ctx, n, S):
    """n = 7 has one prefix (shards 1 and 2 empty), n = 8 seven (3/2/2 over
    three shards, one empty shard of eight)."""
    rng = np.random.default_rng(9300 + 10 * n + S)
    for lattice in (False, True):
        d = _cities_matrix(n, rng, lattice)
        for mode in ("chain", "run_all"):
            nodes, depth = _check(gpu_ctx, d, S, mode)
            assert sum(nodes) == _enum_nodes(n) and depth == n - 7


def _lattice10():
    xy = [(x, y) for x in range(3) for y in range(3)] + [(1.0, 0.5)]
    return O.distance_matrix([(i, float(x), float(y)) for i, (x, y) in enumerate(xy)])


def test_tied_optima_tie_key_without_records(gpu_ctx, knobs):
    """Thousands of tied optima, a 2-record buffer per shard: the shards' tie
    keys answer, no record is read."""
    d = _lattice10()
    knobs.set("SEARCH_RECORD_CAP", "2")
    shards, _ = _open(gpu_ctx, d, 2)
    try:
        _run(shards, "chain")
        cost, tour, by_key = _winner(gpu_ctx, d, shards)
        assert by_key and (cost, tour) == _oracle(d)
        assert sum(X.counters()[1] for X in shards) == _enum_nodes(10)
    finally:
        _close(shards)


def test_tied_optima_lost_records_second_phase(gpu_ctx, knobs):
    """... and without the device tie rule the records overflow: the shards
    run again with the optimum as the bound into buffers of the needed size,
    every optimal record comes back, and the node counters are cumulative.

    The buffer holds ONE record per shard here: the heuristic's bound is
    already the optimum on this instance, so a shard records only the tours
    that tie with it bit for bit, and with two records per shard (the cap that
    overflows the one-shard enumeration) neither of the two shards lost one
    on an MI355X."""
    d = _lattice10()
    knobs.set("SEARCH_RECORD_CAP", "1")
    knobs.set("SEARCH_TIE", "0")
    shards, _ = _open(gpu_ctx, d, 2)
    try:
        _run(shards, "chain")
        opt = min(X.counters()[0] for X in shards)
        print("n = 10 lattice, records claimed per shard:", [X.counters()[2] for X in shards])
        assert all(X.tie_slot(opt)[3] for X in shards)  # no tie key: "overflow"
        lost = 0
        for X in shards:
            try:
                X.records(opt)
            except tspgpu.TspGpuError as e:
                assert e.code == -errno.EOVERFLOW
                lost += 1
        assert lost >= 1
        for X in shards:
            X.reset_records(int(min(max(X.counters()[2], 1 << 16), 1 << 22)))
            X.set_bound(tspgpu.bits_cost(opt, X.dtype))
            X.run_all()
        assert sum(X.counters()[1] for X in shards) == 2 * _enum_nodes(10)
        cost, tour, by_key = _winner(gpu_ctx, d, shards, use_records=True)
        assert not by_key and (cost, tour) == _oracle(d)
    finally:
        _close(shards)


@pytest.mark.parametrize("S", [2, 3, 7])
def test_13_cities_sharded(gpu_ctx, S):
    """One random and one lattice f64 instance and one int32 matrix: each shard
    one chained launch with zero hooks."""
    rng = np.random.default_rng(9100 + 13)
    ds = [_cities_matrix(13, rng, False), _cities_matrix(13, rng, True)]
    m = np.triu(rng.integers(1, 1001, size=(13, 13)).astype(np.int32), 1)
    ds.append(m + m.T)
    for d in ds:
        nodes, depth = _check(gpu_ctx, d, S, "chain")
        assert sum(nodes) == _enum_nodes(13) and depth == 6


@pytest.mark.parametrize("n,enum_off", [(9, True), (6, False)])
def test_round_kernels_with_the_bound_off(gpu_ctx, knobs, n, enum_off):
    """Where the enumeration kernel is not used (knob ENUM_KERNEL=0, n < 7) the
    shard runs the round kernels without the bound: no chain, start / step."""
    if enum_off:
        knobs.set("ENUM_KERNEL", "0")
    rng = np.random.default_rng(9400 + n)
    for lattice in (False, True):
        d = _cities_matrix(n, rng, lattice)
        nodes, _ = _check(gpu_ctx, d, 2, "steps")
        assert sum(nodes) >= math.factorial(n - 1)


def test_one_shard_through_the_flag_equals_the_one_shot(gpu_ctx):
    rng = np.random.default_rng(9100 + 12)
    for lattice in (False, True):
        d = _cities_matrix(12, rng, lattice)
        c1, t1, st = tspgpu.search_solve(gpu_ctx, d, exhaustive=True)
        shards, _ = _open(gpu_ctx, d, 1)
        try:
            _run(shards, "chain")
            cost, tour, _ = _winner(gpu_ctx, d, shards)
            assert (cost, tour) == (c1, t1.tolist()) == _oracle(d)
            assert shards[0].counters()[1] == st["nodes"] == _enum_nodes(12)
            assert shards[0].depth == st["depth"] == 5 and shards[0].items == st["items"]
        finally:
            _close(shards)


def test_exhaustive_with_the_device_bound_is_refused(gpu_ctx):
    d = _cities_matrix(9, np.random.default_rng(1), False)
    with pytest.raises(tspgpu.TspGpuError) as e:
        tspgpu.Search(gpu_ctx, d, device_bound=True, exhaustive=True)
    assert e.value.code == -errno.EINVAL


def test_16_city_golden_three_shards(gpu_ctx):
    """`./tsp 16 1 1000 1000` (15! = 1.3e12 tours, 15!/6! prefixes: the largest
    index range the kernel supports) over three shards: the reference's golden
    cost and city ids.  Measured on an MI355X: see DESIGN.md, "Sharded
    enumeration"."""
    case = next(c for c in O.load_golden("seed0_blocks.json") if c["n"] == 16 and c["B"] == 1 and c["X"] == 1000)
    cities = [(c[0], O.hexf(c[1]), O.hexf(c[2])) for c in case["cities"][0]]
    d = tspgpu.distance_matrix([cities])[0]

    def too_long(*_):
        raise TimeoutError("the 16-city enumeration took more than 60 s")

    old = signal.signal(signal.SIGALRM, too_long)
    signal.alarm(60)
    try:
        shards, _ = _open(gpu_ctx, d, 3)
        try:
            assert shards[0].items == math.factorial(15) // 720 and shards[0].depth == 9
            _run(shards, "chain")
            cost, tour, _ = _winner(gpu_ctx, d, shards)
            nodes = sum(X.counters()[1] for X in shards)
            print("16-city shard kernel ms:", [round(X.timing()[0], 3) for X in shards])
        finally:
            _close(shards)
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)
    assert cost == O.hexf(case["solutions"][0]["cost_hex"])
    assert [cities[t][0] for t in tour] == case["solutions"][0]["ids"]
    assert nodes == _enum_nodes(16)
