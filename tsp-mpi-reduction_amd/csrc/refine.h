// Launchers of the fixed-end path and window refinement kernels (refine.hip,
// DESIGN.md §6d).  A path problem of w cities (start 0, end w-1 fixed) is K1
// on the folded (w-1) x (w-1) matrix P: P[i][j] = D[i][j] for j >= 1,
// P[i][0] = D[i][w-1] for i >= 1, P[0][0] = 0.  Row w-1 and column 0 of D are
// never read.  Every kernel is memory-bound and indexes with 64-bit element
// offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tspgpu.h"

namespace tspgpu {

// fold: nblocks matrices of w x w -> nblocks of (w-1) x (w-1); vbytes 8 (f64)
// or 4 (int32)
hipError_t launch_paths_fold(int vbytes, const void *dist, int w, int64_t nblocks, void *fold, hipStream_t stream);
// a window's identity-order cost ((D[0][1] + D[1][2]) + ...) + D[w-2][w-1],
// a serial left fold, one lane per window
hipError_t launch_paths_identity_cost(const double *dist, int w, int64_t nblocks, double *old_cost,
                                      hipStream_t stream);
// K1's tour 0,t1..tm,0 -> the path's order 0,t1..tm,w-1, in place, for the
// rows of status 0 (the others stay -1)
hipError_t launch_paths_close(int32_t *order, const int32_t *status, int w, int64_t nblocks, hipStream_t stream);

// window build: windows copies of w consecutive cities, window k from
// path + offset + k * stride, into a packed array (the end cities that
// neighbours share appear in both)
hipError_t launch_refine_gather(const tspgpu_city *path, int64_t offset, int64_t stride, int w, int64_t windows,
                                tspgpu_city *packed, hipStream_t stream);
// apply: window k's interior path[s+1 .. s+m], s = offset + k * stride, becomes
// packed[k*w + tour[k*w + j]] iff status[k] == 0 and cost[k] < old_cost[k];
// gain[k] = old - new or 0, replaced[k] = 1 or 0.  The cities are read from
// the packed copy only, never from the path being written.
hipError_t launch_refine_apply(tspgpu_city *path, int64_t offset, int64_t stride, int w, int64_t windows,
                               const tspgpu_city *packed, const int32_t *tour, const int32_t *status,
                               const double *cost, const double *old_cost, double *gain, int32_t *replaced,
                               hipStream_t stream);

}  // namespace tspgpu
