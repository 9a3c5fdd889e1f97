// Host plan of the 2-opt stage (tspgpu_two_opt_path*, include/tspgpu.h,
// DESIGN.md §6e): the grid's size and the greedy selection of a pass's moves.
// Pure host code, no HIP (built into libtspgpu.so and, with
// host/check_two_opt.cpp, into a stand-alone program under ASan + UBSan: make
// check-two-opt).
#pragma once
#include <cstdint>

namespace tspgpu {

constexpr int kTwoOptMaxRing = 4;
constexpr int kTwoOptMaxGrid = 2048;
constexpr int64_t kTwoOptMaxL = (int64_t)1 << 30;

// The best move of position i as the search kernel reports it: reverse
// positions i+1..j, 0 <= i, i+2 <= j <= L-2, gain > 0.  16 bytes on both sides.
struct TwoOptCand {
    double gain;
    int32_t i, j;
};
static_assert(sizeof(TwoOptCand) == 16, "the search kernel writes 16-byte candidates");

// the largest g with 2*g*g <= L, clamped to [1, 2048]; integer arithmetic
int two_opt_grid(int64_t L);

// One pass's selection.  Sorts cand[0..n) by (gain descending, i ascending),
// a total order as every position reports at most one move, then accepts a
// move iff its edge range [i, j] is disjoint from every accepted one.  The
// accepted moves go to acc_i / acc_j in acceptance order (room for n), their
// swap counts (j - i) / 2 as an exclusive prefix to prefix[0..accepted]
// (room for n + 1), and their gains are added to *gain one by one in that
// order.  -> the number accepted, or -EINVAL: a null pointer, n < 0, a
// candidate outside 0 <= i, i+2 <= j <= L-2, a gain that is not > 0, or two
// candidates of one position and one gain (the order would not be total).
int64_t two_opt_select(TwoOptCand *cand, int64_t n, int64_t L, int32_t *acc_i, int32_t *acc_j, int32_t *prefix,
                       double *gain);

}  // namespace tspgpu
