// Host plan of the Or-opt stage (tspgpu_or_opt_path*, include/tspgpu.h,
// DESIGN.md §6f): the candidate record the search kernel writes and the greedy
// selection of a pass's moves.  Pure host code, no HIP (built into
// libtspgpu.so and, with host/check_or_opt.cpp, into a stand-alone program
// under ASan + UBSan: make check-or-opt).  The grid's size is the 2-opt
// stage's (two_opt_plan.h).
#pragma once
#include <cstdint>

namespace tspgpu {

constexpr int kOrOptMaxSeg = 3;

// The best move of position s as the search kernel reports it: positions
// a..a+k-1 go into edge t, reversed when rev.  kr = k | rev << 2.  24 bytes on
// both sides.
struct OrOptCand {
    double gain;
    int32_t s, a, t, kr;
};
static_assert(sizeof(OrOptCand) == 24, "the search kernel writes 24-byte candidates");

constexpr int32_t or_opt_kr(int k, int rev) { return (int32_t)(k | (rev << 2)); }

// An accepted move as the apply kernels read it: the rotated positions are
// lo+1..hi; how = k | rev << 2 | fwd << 3, fwd set when the segment goes to
// the end of the range (t > h) and clear when it goes to its start.
constexpr int32_t kOrOptFwd = 8;

// One pass's selection.  Sorts cand[0..n) by (gain descending, s ascending),
// a total order as every position reports at most one move, then accepts a
// move iff its edge range [lo, hi] ([a-1, t] when t > h = a+k-1, else [t, h])
// is disjoint from every accepted one.  The accepted moves go to acc_lo /
// acc_hi / acc_how in acceptance order (room for n each), their range lengths
// hi - lo as an exclusive prefix to prefix[0..accepted] (room for n + 1), and
// their gains are added to *gain one by one in that order.  -> the number
// accepted, or -EINVAL: a null pointer, n < 0, max_seg outside 1..3, a
// candidate outside the contract (a gain that is not > 0, k outside
// 1..max_seg, a set bit above rev, rev with k = 1, a < 1, h > L-2, t outside
// 0..L-2 or inside [a-1, h], s at neither end of the segment), or two
// candidates of one position and one gain (the order would not be total).
int64_t or_opt_select(OrOptCand *cand, int64_t n, int64_t L, int max_seg, int32_t *acc_lo, int32_t *acc_hi,
                      int32_t *acc_how, int32_t *prefix, double *gain);

}  // namespace tspgpu
