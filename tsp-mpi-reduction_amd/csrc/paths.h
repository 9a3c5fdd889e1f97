// K1 -> K3 hand-off on the device (tspgpu_reduce_device): the
// block search's outputs as they lie in HBM (cities, tour rows of n+1 local
// indices, statuses) become the block paths the merge kernels read
// (convPathToCityPath, assignment2.h:76-84), together with the facts the host
// front of tspgpu_reduce scans the paths for.
//
// Gather.  paths[b*L + i] = cities[b*n + tour[b*(n+1) + i]] for i < L =
// tspgpu_tour_length(n) (the n == 2 row is [1,0], L = 2), moved as 8-byte
// words.  The row of a block whose status is non-zero is never read.  Every
// entry is checked against [0, n) before it indexes anything: a row with an
// entry outside raises kPathBadIndex and nothing of it is gathered.
//
// Facts, over the gathered cities: the exact minimum and maximum of x and of
// y (order keys of the doubles, so the host's bounding-box diagonal has the
// bits of the host scan's), of id, a non-finite flag, "some path does not
// close on its first city's id", and the first block with a non-zero status
// together with that status.
//
// Id uniqueness (the other half of the one-kernel fold's precondition; each
// block's closing copy left out, as on the host).  When id_max - id_min <
// 8*B*L a bitmap over [id_min, id_max] is filled with atomicOr and a set bit
// met twice raises kPathDupId.  A wider id range raises kPathWideIds instead:
// uniqueness is then not decided and the caller takes the general per-merge
// path, which reproduces mergeBlocks for any input — the same answer, only
// slower.  (The host scan sorts the ids and so decides every range; this is
// the one place where the device form may fold slower than the host form.)
//
// The facts' words and the host's rules over them are paths_facts.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_desc.h"
#include "paths_facts.h"
#include "tspgpu.h"

namespace tspgpu {

constexpr int kPathsMaxN = TSPGPU_MAX_CITIES;

// d_status may be null (every block valid).  grid_cap: the most workgroups
// (the context's CU count * 8, as the merge kernels' grids).
hipError_t launch_paths_gather(const tspgpu_city *d_cities, const int32_t *d_tour, const int32_t *d_status, int n,
                               int nblocks, tspgpu_city *d_paths, PathFacts *d_facts, int grid_cap,
                               hipStream_t stream);
// behind launch_paths_gather on the same stream; d_bitmap: path_bitmap_bits()
// zeroed bits.  Does nothing when the facts already hold a non-zero status or
// kPathBadIndex (parts of d_paths are unwritten then).
hipError_t launch_paths_unique(const tspgpu_city *d_paths, int L, int nblocks, uint32_t *d_bitmap,
                               PathFacts *d_facts, int grid_cap, hipStream_t stream);

// The ragged forms (tspgpu_reduce_ragged_device): block b has
// d_desc[b].n cities at d_cities + d_desc[b].city, its tour row starts at
// d_tour + b * tour_stride and its path of d_desc[b].L cities goes to d_paths
// + d_desc[b].path (block_desc.h; the caller guarantees 2 <= n <= kPathsMaxN,
// L = tspgpu_tour_length(n) <= tour_stride).  Same facts, same two ordering
// guarantees.  total: all gathered cities (<= INT_MAX); d_bitmap:
// path_bitmap_bits_total(total) zeroed bits, whole words.  "Closing copy" is
// the last city of a block's path.
hipError_t launch_paths_gather_ragged(const tspgpu_city *d_cities, const int32_t *d_tour, int tour_stride,
                                      const int32_t *d_status, const BlockDesc *d_desc, int nblocks,
                                      tspgpu_city *d_paths, PathFacts *d_facts, int grid_cap, hipStream_t stream);
hipError_t launch_paths_unique_ragged(const tspgpu_city *d_paths, const BlockDesc *d_desc, int nblocks,
                                      unsigned long long total, uint32_t *d_bitmap, PathFacts *d_facts, int grid_cap,
                                      hipStream_t stream);

}  // namespace tspgpu
