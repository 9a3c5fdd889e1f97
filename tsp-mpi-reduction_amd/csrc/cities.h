// Launchers of the device distance build (cities.hip): city
// coordinates in, the reference's distance matrices out, bit for bit, with
// the host's pow consulted only for the squares dist_exact.h flags.
//
//   build   squares of every coordinate difference into the matrix itself
//           (x-square at d[i][j], y-square at d[j][i], i < j), the flagged
//           ones also appended to the fix-up list
//   patch   the host's pow results into the flagged slots
//   finish  d[i][j] = d[j][i] = sqrt_rn(d[i][j] + d[j][i])
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_desc.h"
#include "tspgpu.h"

namespace tspgpu {

constexpr int kCitiesMaxN = TSPGPU_MAX_CITIES;

// The fix-up list (device): entry t is the matrix element fix_slot[t] (an
// index into the whole dist array) whose square is pow(fix_dx[t], 2).
// *fix_count (zeroed by the caller) ends as the number of flagged squares,
// which may exceed fix_cap: entries past fix_cap are not stored.
hipError_t launch_cities_build(const tspgpu_city *cities, int n, int nblocks, double *dist, int64_t *fix_slot,
                               double *fix_dx, unsigned long long fix_cap, unsigned long long *fix_count,
                               hipStream_t stream);
// dist[fix_slot[t]] = fix_val[t] for t < count
hipError_t launch_cities_patch(double *dist, const int64_t *fix_slot, const double *fix_val,
                               unsigned long long count, hipStream_t stream);
hipError_t launch_cities_finish(int n, int nblocks, double *dist, hipStream_t stream);

// The ragged forms: block b's n, cities and matrix are
// desc[b]'s (device table; an entry with n = 0 is skipped); fix_slot indexes
// the whole packed dist array as above.  Every desc[b].n must be in
// [0, kCitiesMaxN] (the caller checks: the kernels stage a block in LDS rows
// of kCitiesMaxN).
hipError_t launch_cities_build_ragged(const tspgpu_city *cities, const BlockDesc *desc, int nblocks, double *dist,
                                      int64_t *fix_slot, double *fix_dx, unsigned long long fix_cap,
                                      unsigned long long *fix_count, hipStream_t stream);
hipError_t launch_cities_finish_ragged(const BlockDesc *desc, int nblocks, double *dist, hipStream_t stream);

}  // namespace tspgpu
