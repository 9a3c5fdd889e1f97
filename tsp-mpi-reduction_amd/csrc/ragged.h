// Launchers of the two ragged-batch kernels (ragged.hip): the gather that
// validates every block while it moves it into its size bucket, and the
// scatter that puts costs and tours back in caller order with a status per
// block.  The layout is the host plan's (ragged_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include "ragged_plan.h"

namespace tspgpu {

// vbytes 8: f64 values, 4: int32.  desc / status: nblocks entries (device).
// src + desc[b].src must hold n*n readable elements for every block with
// pre == 0; stage_dist is the plan's dist staging (dist_elems elements).
hipError_t launch_ragged_gather(int vbytes, const void *src, const RaggedDesc *desc, int nblocks, void *stage_dist,
                                int32_t *stage_status, hipStream_t stream);
// cost_out: nblocks values; tour_out: nblocks rows of tour_stride entries;
// status_out: nblocks codes.
hipError_t launch_ragged_scatter(int vbytes, const RaggedDesc *desc, const int32_t *stage_status, int nblocks,
                                 const void *stage_cost, const int32_t *stage_tour, void *cost_out,
                                 int32_t *tour_out, int tour_stride, int32_t *status_out, hipStream_t stream);

}  // namespace tspgpu
