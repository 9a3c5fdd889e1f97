// Launchers of the Or-opt stage's own kernels (or_opt.hip; the contract is in
// include/tspgpu.h "Or-opt with a neighbour grid", the design in DESIGN.md
// §6f).  The state (ord, pos, px, py), the grid and their kernels are the
// 2-opt stage's: two_opt.h says what each array holds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "or_opt_plan.h"
#include "two_opt.h"

namespace tspgpu {

// the best move of every position 1 .. L-2 -> cand[atomicAdd(count, 1)] (count
// zeroed by the caller; at most L - 2 candidates); max_seg 1..3 picks the
// instantiation
hipError_t launch_or_opt_search(int L, int g, int ring, int max_seg, const int32_t *ord, const int32_t *pos,
                                const double *px, const double *py, const int32_t *cell, const int32_t *start,
                                const double *cell_x, const double *cell_y, const int32_t *cell_city,
                                OrOptCand *cand, uint32_t *count, hipStream_t stream);
// moves disjoint rotations: move m rotates positions acc_lo[m]+1 .. acc_hi[m]
// as acc_how[m] says (or_opt_plan.h); prefix[0..moves] the exclusive prefix of
// their lengths hi - lo, total = prefix[moves] < L.  Two kernels: stage
// gathers the new ord / px / py of every rotated position into s_ord / s_x /
// s_y (L each), commit writes them back and updates pos.
hipError_t launch_or_opt_apply(int moves, const int32_t *acc_lo, const int32_t *acc_hi, const int32_t *acc_how,
                               const int32_t *prefix, int total, int L, int32_t *ord, int32_t *pos, double *px,
                               double *py, int32_t *s_ord, double *s_x, double *s_y, hipStream_t stream);

}  // namespace tspgpu
