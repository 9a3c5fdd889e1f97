// One block of a PACKED ragged batch: block b has n[b] cities
// at cities + sum_{a<b} n[a], its matrix at dist + sum n[a]^2 and its path of
// L[b] cities at paths + sum L[a].  The host takes the prefix sums and uploads
// the table; the ragged kernels of cities.hip (city, dist, n), paths.hip
// (city, path, n, L) and merge.hip's fold (path, L) read a block's entry where
// their uniform siblings compute b*n, b*n*n and b*L.
#pragma once
#include <stdint.h>

namespace tspgpu {

struct BlockDesc {
    int64_t city;  // first city of the block in the packed city array
    int64_t dist;  // first element of its matrix in the packed matrices
    int64_t path;  // first city of its path in the packed paths
    int32_t n;     // cities (0: the distance build skips the block)
    int32_t L;     // cities of its path
};
static_assert(sizeof(BlockDesc) == 32, "BlockDesc is uploaded as is");

}  // namespace tspgpu
