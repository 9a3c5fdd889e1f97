"""tests/golden/wide_large.json (n = 23 .. 26, made by
tests/golden/make_wide_golden.py from the CPU oracle): the stored answers are
self-consistent and tied to the oracle.  The GPU side is
tests/test_wide_large_gpu.py."""
import numpy as np
import pytest

import oracle_py as O

DATA = O.load_golden("wide_large.json")
IDS = [f"n{i['n']}-{i['kind']}" for i in DATA]


def matrix(inst):
    """The float64 matrix the oracle solved."""
    if inst["kind"] == "integer":
        return np.array(inst["matrix"], dtype=np.int32).astype(np.float64)
    return O.distance_matrix([(c, O.hexf(x), O.hexf(y)) for c, x, y in inst["cities"]])


def left_fold(d, tour):
    """((d[0][t1] + d[t1][t2]) + ...) + d[t_{n-1}][0]: how the DP accumulates
    the cost of its own tour (oracle.c: G[S][k] = G[S\\k][m] + d[m][k])."""
    acc = d[tour[0], tour[1]]
    for a, b in zip(tour[1:-1], tour[2:]):
        acc = acc + d[a, b]
    return acc


def test_file_has_every_size_and_kind():
    assert {(i["n"], i["kind"]) for i in DATA} >= {(n, k) for n in (23, 24, 25)
                                                   for k in ("uniform", "lattice", "integer")}
    for inst in DATA:
        assert float(inst["cost"]) == O.hexf(inst["cost_hex"])
        if inst["kind"] == "integer":
            m = np.array(inst["matrix"])
            assert m.shape == (inst["n"], inst["n"]) and not m.diagonal().any()
            off = m[~np.eye(inst["n"], dtype=bool)]
            assert off.min() >= 1 and off.max() <= 1000 and (m != m.T).any()
        else:
            assert len(inst["cities"]) == inst["n"]


@pytest.mark.parametrize("inst", DATA, ids=IDS)
def test_tour_is_a_permutation_and_folds_to_the_cost(inst):
    n, tour = inst["n"], inst["tour"]
    assert len(tour) == n + 1 and tour[0] == 0 and tour[-1] == 0
    assert sorted(tour[1:-1]) == list(range(1, n))
    got = left_fold(matrix(inst), tour)
    assert float(got).hex() == inst["cost_hex"]


@pytest.mark.parametrize("inst", [i for i in DATA if i["n"] == 23], ids=[s for s in IDS if s.startswith("n23-")])
def test_oracle_returns_the_stored_answer(inst):
    cost, tour = O.solve_block(matrix(inst))
    assert float(cost).hex() == inst["cost_hex"] and tour == inst["tour"]
