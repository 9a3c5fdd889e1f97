"""2-opt with a neighbour grid on the GPU where the grid's scan leaves one
workgroup, on cell borders and at extreme scales (tspgpu_two_opt_path*,
DESIGN.md §6e), against the Python model (tests/two_opt_model.py), bit for bit
as tests/test_two_opt_gpu.py compares: path ids and coordinate bits, passes,
candidates and moves equal, `gain` as bits.

What each input reaches, and that a wrong implementation gives another result
on it, is asserted on the CPU in tests/test_two_opt_model.py:
  sweep-2178               g = 33: two scan workgroups, the last one ragged, a non-zero sums[] added
  sweep-8712-ring3         g = 66: five scan workgroups; ring 3
  sweep-526338-ring1-cut3  g = 513: 258 first-level workgroups, two items per lane in the second level;
                           about 41000 moves and 149000 candidates in three passes
  cell-edges-242           coordinates on and beside the cell borders: the rounding of the cell formula
  scrambled-400-x2^E       sqrt_rn's scaled branch (2^-500), subnormal squares (2^-520), sums near 2^1023 (2^500)
  minus-zero-min           both minima written as -0.0 and as +0.0

Wall times measured on an MI355X machine, in one process with
tests/test_two_opt_gpu.py, 7.7 s for both files, about 5.9 s of it here
(pytest's per-test durations; a test that is first to ask for an input also
pays for its model result, computed once per process):
  test_inputs_match_the_model[sweep-526338-ring1-cut3]   2.84 s (model included)
  test_inputs_match_the_model[sweep-8712-ring3]          1.67 s (model included)
  test_a_large_grid_then_small_ones_then_growth_again    0.44 s (all five model results cached)
  test_the_range_limit_is_the_models                     0.13 s
  test_inputs_match_the_model[sweep-2178]                0.12 s
  test_inputs_match_the_model[scrambled-400-x2^E]        0.10 - 0.11 s each
  test_scaled_inputs_keep_the_unscaled_order             0.07 s
  test_inputs_match_the_model[cell-edges-242]            0.03 s (+ 0.23 s making the session's context)
  test_fill_order_does_not_matter                        0.02 s
  test_host_form_equals_device_form, minus-zero-min      0.01 s or less each
"""
import errno

import pytest

import tspgpu
import two_opt_model as T
from test_two_opt_gpu import check_model, on_device, same_path, same_stats

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(T.SCALE_INPUTS))
def test_inputs_match_the_model(gpu_ctx, name):
    path, got, stats = check_model(gpu_ctx, name)
    assert stats["moves"] >= 1 and got[0] == path[0] and got[-1] == path[-1]
    assert stats["passes"] <= T.built(name)[2]


@pytest.mark.parametrize("name", ["sweep-2178", "cell-edges-242"])
def test_host_form_equals_device_form(gpu_ctx, name):
    path, ring, passes, want, wstats = T.solved(name)
    stats, got = on_device(gpu_ctx, path, ring, passes)
    assert same_stats(stats, wstats) and same_path(got, want)


def test_fill_order_does_not_matter(gpu_ctx):
    """The cities of a cell lie in the order the fill kernel's atomics gave
    them; two runs on one context agree with each other (and the model)."""
    path, ring, passes, want, wstats = T.solved("sweep-2178")
    first, stats1 = gpu_ctx.two_opt_path(list(path), ring, passes)
    second, stats2 = gpu_ctx.two_opt_path(list(path), ring, passes)
    assert same_path(first, second) and same_stats(stats1, stats2)
    assert same_path(first, want) and same_stats(stats1, wstats)


def test_scaled_inputs_keep_the_unscaled_order(gpu_ctx):
    base, ring, passes = T.built(T.SCALED_BASE)
    unscaled, ustats = gpu_ctx.two_opt_path(list(base), ring, passes)
    for name in sorted(T.SCALED_INPUTS):
        got, stats = gpu_ctx.two_opt_path(list(T.built(name)[0]), ring, passes)
        assert [c[0] for c in got] == [c[0] for c in unscaled]
        assert all(stats[k] == ustats[k] for k in ("passes", "candidates", "moves"))


def test_the_range_limit_is_the_models(gpu_ctx):
    """The two neighbours of the -ERANGE limit: refused with the path left as
    it was on one side, the model's result on the other."""
    base = list(T.built(T.SCALED_BASE)[0])
    for exponent, code in T.RANGE_EDGE:
        path = T.scaled(base, exponent)
        want, wstats = T.two_opt(path)
        rc, after = on_device(gpu_ctx, path, 2, 1000)
        if code:
            assert want is None and wstats == code == -errno.ERANGE
            assert rc == code and same_path(after, path)
            with pytest.raises(tspgpu.TspGpuError) as err:
                gpu_ctx.two_opt_path(path)
            assert err.value.code == code
        else:
            assert same_stats(rc, wstats) and same_path(after, want) and wstats["moves"] >= 1
            got, stats = gpu_ctx.two_opt_path(path)
            assert same_stats(stats, wstats) and same_path(got, want)
    check_model(gpu_ctx, "scrambled-400-cut3")  # the context still works


def test_a_large_grid_then_small_ones_then_growth_again():
    """One fresh context: the largest grid first, then grids inside one scan
    workgroup over buffers (start, sums, cursor) that held the larger one,
    then growth past one workgroup again."""
    ctx = tspgpu.Context(device=0)
    try:
        for name in ("sweep-526338-ring1-cut3", "sweep-2178", "L4", "lattice-scrambled-200", "sweep-8712-ring3"):
            check_model(ctx, name)
    finally:
        ctx.close()
