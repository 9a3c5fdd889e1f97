// Host plan of a ragged K1 batch (tspgpu_solve_ragged*, include/tspgpu.h):
// blocks of different city counts, sorted into one contiguous bucket per
// size so that every bucket is a plain K1 launch.  Pure host code, no HIP
// (built into libtspgpu.so and, with host/check_ragged.cpp, into a stand-alone
// program under ASan + UBSan: make check-ragged).
//
// Staging layout (element offsets; V = the value type, 8 or 4 bytes):
//   dist   bucket n at dist_base[n] (a multiple of 256 bytes), its blocks
//          contiguous at n*n elements in caller order
//   cost   bucket n at cost_base[n] (V elements, 256-byte multiple), one per block
//   tour   bucket n at tour_base[n] (int32 entries, 256-byte multiple), n+1 per block
// which is what K1 takes for (dist, cost, tour) of nblocks = count[n] blocks.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tspgpu {

constexpr int kRaggedMinN = 2;
constexpr int kRaggedMaxN = 20;          // TSPGPU_MAX_CITIES
constexpr int kRaggedStrictMaxN = 16;    // TSPGPU_REFERENCE_MAX_CITIES
constexpr size_t kRaggedAlignBytes = 256;

// One block for the gather and scatter kernels (ragged.hip).  A block the
// plan refuses (pre != 0) is in no bucket: n = 0 and every offset is 0, its
// matrix is never read.
struct RaggedDesc {
    int64_t src;   // element offset of the matrix in the caller's array
    int64_t dst;   // element offset of the block's slot in the dist staging
    int64_t tour;  // entry offset of the block's tour in the tour staging
    int32_t cost;  // element index of the block's cost in the cost staging
    int16_t n;     // cities (0: refused)
    int16_t pre;   // 0, or -EINVAL from the plan
};
static_assert(sizeof(RaggedDesc) == 32, "RaggedDesc is uploaded as is");

struct RaggedPlan {
    int nblocks = 0;
    int max_n = 0;                            // largest in-range n (0: none)
    int in_range = 0;                         // blocks in buckets
    int64_t ext_lo = 0, ext_hi = 0;           // covering extent [lo, hi) in elements (0, 0: none)
    int count[kRaggedMaxN + 1] = {};          // blocks of bucket n
    int begin[kRaggedMaxN + 1] = {};          // bucket n = order[begin[n] .. begin[n] + count[n])
    int64_t dist_base[kRaggedMaxN + 1] = {};  // staging offsets of bucket n (elements / entries)
    int64_t cost_base[kRaggedMaxN + 1] = {};
    int64_t tour_base[kRaggedMaxN + 1] = {};
    int64_t dist_elems = 0, cost_elems = 0, tour_elems = 0;  // staging sizes
    std::vector<int32_t> pre;       // per block: 0 or -EINVAL
    std::vector<int32_t> slot;      // per block: position within its bucket (-1: refused)
    std::vector<int32_t> order;     // in-range blocks sorted by n, stable
    std::vector<RaggedDesc> desc;   // per block, caller order
};

// Fills *plan.  vbytes: 8 or 4.  Returns 0, or -EINVAL (n/offset NULL with
// nblocks > 0, nblocks < 0, vbytes neither 8 nor 4, or a staging index beyond
// what RaggedDesc holds).  Bad blocks are no error: they get pre = -EINVAL.
int ragged_plan(const int32_t *n, const int64_t *offset, int nblocks, int strict, int vbytes, RaggedPlan *plan);

}  // namespace tspgpu
