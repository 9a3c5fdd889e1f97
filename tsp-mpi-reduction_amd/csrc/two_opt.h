// Launchers of the 2-opt stage's kernels (two_opt.hip; the contract is in
// include/tspgpu.h "2-opt with a neighbour grid", the design in DESIGN.md §6e).
//
// Supported L <= 2^30 (kTwoOptMaxL): positions, cities, cells and candidate
// slots are int32.  Only the 8-byte words of the city arrays (3 L of them) can
// pass 2^31 and are indexed in 64 bits.
//
// State, all by position unless named otherwise:
//   ord[pos] the city there (its index in the input), pos[city] its inverse,
//   px[pos], py[pos] that city's coordinates.
// Grid (built once; cities do not move): cell[city] = cy * g + cx, start[c]
// the first slot of cell c in the cell-sorted arrays cell_x, cell_y,
// cell_city (start[g*g] = L); the order inside a cell is whatever the fill
// kernel's atomics gave, and no result depends on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tspgpu.h"
#include "two_opt_plan.h"

namespace tspgpu {

// what the bounds kernel leaves for the host: the least and greatest x and y
// as order-preserving integers (two_opt_decode) and a non-finite flag
struct TwoOptBounds {
    unsigned long long xmin, xmax, ymin, ymax, nonfinite;
};
// before launch_two_opt_bounds
TwoOptBounds two_opt_bounds_init();
double two_opt_decode(unsigned long long key);

// path -> px, py, ord = pos = identity, and the bounds (atomics on *bounds)
hipError_t launch_two_opt_bounds(const tspgpu_city *path, int L, double *px, double *py, int32_t *ord, int32_t *pos,
                                 TwoOptBounds *bounds, hipStream_t stream);
// cell[city] and count[cell] += 1 (count zeroed by the caller); x, y by city
hipError_t launch_two_opt_cells(const double *x, const double *y, int L, double xmin, double ex, double ymin,
                                double ey, int g, int32_t *cell, int32_t *count, hipStream_t stream);
// start[0..cells) = the exclusive prefix of count[0..cells) (in place
// allowed), start[cells] = total, the sum of all counts, which the caller
// knows; sums: room for (cells + 1023) / 1024 int32
hipError_t launch_two_opt_scan(const int32_t *count, int cells, int32_t total, int32_t *start, int32_t *sums,
                               hipStream_t stream);
// the cell-sorted arrays (cursor: cells int32, zeroed by the caller)
hipError_t launch_two_opt_fill(const double *x, const double *y, const int32_t *cell, int L, const int32_t *start,
                               int32_t *cursor, double *cell_x, double *cell_y, int32_t *cell_city,
                               hipStream_t stream);
// the best move of every position -> cand[atomicAdd(count, 1)] (count zeroed
// by the caller; at most L - 3 candidates)
hipError_t launch_two_opt_search(int L, int g, int ring, const int32_t *ord, const int32_t *pos, const double *px,
                                 const double *py, const int32_t *cell, const int32_t *start, const double *cell_x,
                                 const double *cell_y, const int32_t *cell_city, TwoOptCand *cand, uint32_t *count,
                                 hipStream_t stream);
// moves disjoint reversals: move m reverses positions acc_i[m]+1 .. acc_j[m];
// prefix[0..moves] the exclusive prefix of their swap counts (j - i) / 2
hipError_t launch_two_opt_apply(int moves, const int32_t *acc_i, const int32_t *acc_j, const int32_t *prefix, int swaps,
                                int32_t *ord, int32_t *pos, double *px, double *py, hipStream_t stream);
// out[pos] = in[ord[pos]]; in and out must not overlap
hipError_t launch_two_opt_emit(const tspgpu_city *in, const int32_t *ord, int L, tspgpu_city *out, hipStream_t stream);

}  // namespace tspgpu
