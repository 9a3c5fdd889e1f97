"""search_dist.solve_sharded(..., exhaustive=True): the exhaustive enumeration
over the ranks of a gloo group.

CPU part: the driver's logic with a brute-force stand-in for an exhaustive
tspgpu.Search (its chain runs the whole shard and calls the hook zero times).
GPU part (-m gpu): the real enumeration kernel, two ranks sharing device 0.
"""
import os
import sys

import numpy as np
import pytest

from test_search_dist import ROOT, FakeSearch, _lattice, _run


class FakeEnumSearch(FakeSearch):
    """FakeSearch as an exhaustive shard: takes `exhaustive`, no device bound,
    and chain() folds every tour of the shard without a single hook."""

    def __init__(self, ctx, dist, shard=0, nshards=1, depth=0, device_bound=False, exhaustive=False):
        assert exhaustive and not device_bound
        super().__init__(ctx, dist, shard=shard, nshards=nshards, depth=depth)

    def chain(self, exchange_every=0, hook=None, native_hook=None):
        assert native_hook is None  # (gloo)
        self.run_all()
        return True


def _cpu_worker(rank, world, port, dist, cap, tie_on, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tsp-mpi-reduction_amd")]
    import torch.distributed as tdist

    import search_dist

    FakeEnumSearch.cap = cap
    FakeEnumSearch.tie_on = tie_on
    search_dist.tspgpu.Search = FakeEnumSearch
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    cost, tour, st = search_dist.solve_sharded(None, dist, exhaustive=True)
    out.put((rank, cost, tour.tolist(), st["phases"], st["nodes"], st["tie"], st["record_gather"], st["exchanges"],
             st["hooks"], st["exhaustive"], st["bound"]))
    tdist.destroy_process_group()


@pytest.mark.parametrize("world,cap,tie_on", [(2, 1 << 30, True), (3, 1 << 30, True), (2, 1, False)])
def test_exhaustive_driver_cpu(world, cap, tie_on):
    """Every rank returns the oracle's cost and tour on tie-heavy 7-city
    lattices; no in-chain exchange, one exchange after the chains, every tour
    folded once (720 nodes) — twice when the records were lost and the second
    phase re-enumerates with the optimum as the bound."""
    import oracle_py as O

    for seed in (5 + world, 11, 12):
        d = _lattice(7, seed)
        res = _run(_cpu_worker, world, d, cap, tie_on)
        oc, ot = O.solve_block(d)
        assert len(res) == world
        for rank, cost, tour, phases, nodes, tie, gathered, exchanges, hooks, exhaustive, bound in res:
            assert cost == oc and tour == ot
            assert hooks == 0 and exchanges == 1
            assert exhaustive is True and bound == "host"
            if tie_on:
                assert phases == 1 and nodes == 720 and tie == 1 and gathered == 0
            else:
                assert phases == 2 and nodes == 1440 and tie == 0 and gathered == 1


def test_exhaustive_rejects_the_device_bound():
    import search_dist

    with pytest.raises(ValueError):
        search_dist.solve_sharded(None, _lattice(7, 11), exhaustive=True, bound="device")


def _enum_nodes(n):
    import math
    N = n - 1
    return sum(math.factorial(N) // math.factorial(N - l) for l in range(1, N + 1))


def _gpu_worker(rank, world, port, dist, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tsp-mpi-reduction_amd")]
    import torch.distributed as tdist

    import search_dist
    import tspgpu

    tdist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = tspgpu.Context(device=0)
    res = []
    for d in dist:
        cost, tour, st = search_dist.solve_sharded(ctx, d, exhaustive=True)
        res.append((cost, tour.tolist(), st["rank_nodes"], st["nodes"], st["exchanges"], st["phases"], st["tie"],
                    st["record_gather"], st["chained"], st["hooks"], st["exhaustive"]))
    ctx.close()
    out.put((rank, res))
    tdist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_enumerate_on_one_gpu():
    """Two processes, one GPU, gloo: each rank's shard is one enumeration
    launch; the winner from the gathered tie keys (one phase, no record
    gather), the node total exactly every partial path."""
    import oracle_py as O

    rng = np.random.default_rng(9213)
    ds = []
    for lattice in (False, True):
        xy = rng.integers(0, 4, size=(13, 2)).astype(np.float64) if lattice else rng.uniform(0, 1000, size=(13, 2))
        ds.append(O.distance_matrix([(i, xy[i, 0], xy[i, 1]) for i in range(13)]))
    res = _run(_gpu_worker, 2, ds)
    for k, d in enumerate(ds):
        oc, ot = O.solve_block(d)
        r0, r1 = res[0][1][k], res[1][1][k]
        for cost, tour, *_ in (r0, r1):
            assert cost == oc and tour == ot
        assert r0[3] == r1[3] == _enum_nodes(13) == r0[2] + r1[2]
        for r in (r0, r1):
            assert r[4] == 1 and r[5] == 1 and r[6] == 1 and r[7] == 0 and r[8] == 1 and r[9] == 0 and r[10], r
