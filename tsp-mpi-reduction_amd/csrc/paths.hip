// K1 -> K3 hand-off kernels (paths.h): gather the block paths
// from the block search's device outputs, with the facts the merge needs, and
// decide id uniqueness with a bitmap.
//
// Gather gives a 64-lane wave to a group of whole tour rows: a row is 3*L
// 8-byte words (at most 63), so a wave holds floor(64 / (3*L)) rows and every
// lane moves one word of one city per step; a row's words are contiguous in
// the output, so the stores coalesce.  Holding whole rows lets one ballot
// decide "this row has an entry outside [0, n)" before any lane of the row
// indexes the cities.  Built without the K1 kernels' -fno-honor-nans: a NaN
// coordinate must raise the non-finite flag.
#include "paths.h"

namespace tspgpu {
namespace {

constexpr int kPtThreads = 256;
constexpr int kPtWaves = kPtThreads / 64;

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m)
{
    const int lo = __shfl_xor((int)(unsigned)v, m), hi = __shfl_xor((int)(unsigned)(v >> 32), m);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// what a lane, then a wave, then a workgroup has seen
struct Seen {
    unsigned long long xmin, xmax, ymin, ymax;
    int id_min, id_max;
    unsigned flags;
};
__device__ __forceinline__ void seen_join(Seen &a, const Seen &b)
{
    a.xmin = b.xmin < a.xmin ? b.xmin : a.xmin;
    a.xmax = b.xmax > a.xmax ? b.xmax : a.xmax;
    a.ymin = b.ymin < a.ymin ? b.ymin : a.ymin;
    a.ymax = b.ymax > a.ymax ? b.ymax : a.ymax;
    a.id_min = b.id_min < a.id_min ? b.id_min : a.id_min;
    a.id_max = b.id_max > a.id_max ? b.id_max : a.id_max;
    a.flags |= b.flags;
}

// what the lanes have seen -> the facts: wave, then workgroup, then one
// guarded atomic per word (reached by every thread of the workgroup)
__device__ __forceinline__ void seen_publish(Seen s, Seen *wseen, int lane, int wave, PathFacts *__restrict__ facts)
{
#pragma unroll
    for (int o = 1; o < 64; o *= 2) {
        Seen q;
        q.xmin = shfl_xor_u64(s.xmin, o);
        q.xmax = shfl_xor_u64(s.xmax, o);
        q.ymin = shfl_xor_u64(s.ymin, o);
        q.ymax = shfl_xor_u64(s.ymax, o);
        q.id_min = __shfl_xor(s.id_min, o);
        q.id_max = __shfl_xor(s.id_max, o);
        q.flags = (unsigned)__shfl_xor((int)s.flags, o);
        seen_join(s, q);
    }
    if (lane == 0) wseen[wave] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kPtWaves; ++w) seen_join(s, wseen[w]);
    if (s.xmin != ~0ull) atomicMin(&facts->xmin, s.xmin);
    if (s.xmax != 0ull) atomicMax(&facts->xmax, s.xmax);
    if (s.ymin != ~0ull) atomicMin(&facts->ymin, s.ymin);
    if (s.ymax != 0ull) atomicMax(&facts->ymax, s.ymax);
    if (s.id_min <= s.id_max) {
        atomicMin(&facts->id_min, s.id_min);
        atomicMax(&facts->id_max, s.id_max);
    }
    if (s.flags) atomicOr(&facts->flags, s.flags);
}

__global__ __launch_bounds__(kPtThreads) void paths_gather_kernel(const tspgpu_city *__restrict__ cities,
                                                                 const int32_t *__restrict__ tour,
                                                                 const int32_t *__restrict__ status, int n, int L,
                                                                 int nblocks, int rows_per_wave,
                                                                 tspgpu_city *__restrict__ paths,
                                                                 PathFacts *__restrict__ facts)
{
    static_assert(sizeof(tspgpu_city) == 24, "City layout");
    __shared__ Seen wseen[kPtWaves];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpr = 3 * L;         // words of a row
    const int r = lane / wpr;      // this lane's row of the wave's group
    const int j = lane - r * wpr;  // its word of the row: city i, word f
    const int i = j / 3, f = j - 3 * i;
    const bool mine = r < rows_per_wave;
    const unsigned long long rowmask = mine ? ((1ull << wpr) - 1ull) << (r * wpr) : 0ull;
    Seen s{~0ull, 0ull, ~0ull, 0ull, INT_MAX, INT_MIN, 0u};
    const long long groups = ((long long)nblocks + rows_per_wave - 1) / rows_per_wave;
    // (the trip count is wave-uniform: every lane reaches the ballot)
    for (long long g = (long long)blockIdx.x * kPtWaves + wave; g < groups; g += (long long)gridDim.x * kPtWaves) {
        const long long b = g * rows_per_wave + r;
        const bool live = mine && b < nblocks;
        int st = 0;
        if (live && status) st = status[b];
        if (live && st != 0 && j == 0)
            atomicMin(&facts->first_bad, ((unsigned long long)b << 32) | (unsigned long long)(unsigned)st);
        const bool read = live && st == 0;  // (a bad block's tour row is never read)
        int t = 0;
        if (read) t = tour[b * (n + 1) + i];
        const bool bad = read && (t < 0 || t >= n);
        const bool rowbad = (__builtin_amdgcn_ballot_w64(bad) & rowmask) != 0ull;
        if (rowbad) s.flags |= kPathBadIndex;
        if (read && !rowbad) {
            const unsigned long long *src = reinterpret_cast<const unsigned long long *>(cities + (b * n + t));
            const unsigned long long w = src[f];
            reinterpret_cast<unsigned long long *>(paths + (b * L + i))[f] = w;
            if (f == 0) {
                const int id = (int)(unsigned)w;
                s.id_min = id < s.id_min ? id : s.id_min;
                s.id_max = id > s.id_max ? id : s.id_max;
                if (i == L - 1) {
                    // (entry 0 of this row passed the range check above)
                    const int id0 = cities[b * n + tour[b * (n + 1)]].id;
                    if (id != id0) s.flags |= kPathOpen;
                }
            } else {
                const double v = __builtin_bit_cast(double, w);
                if (!__builtin_isfinite(v)) {
                    s.flags |= kPathNonFinite;
                } else {
                    const unsigned long long k = path_order_key(v);
                    if (f == 1) {
                        s.xmin = k < s.xmin ? k : s.xmin;
                        s.xmax = k > s.xmax ? k : s.xmax;
                    } else {
                        s.ymin = k < s.ymin ? k : s.ymin;
                        s.ymax = k > s.ymax ? k : s.ymax;
                    }
                }
            }
        }
    }
    seen_publish(s, wseen, lane, wave, facts);
}

// The ragged gather: rows of different lengths.  A row gets a
// FIXED group of kPtRowLanes = 21 lanes, one lane per city of the longest
// possible path (tspgpu_tour_length(20)), so a wave holds three rows whatever
// their lengths are (lane 63 idles) and a lane moves the three words of its
// city.  The row masks are constants of the lane, the trip count depends on
// nblocks alone, and every lane reaches the ballot: lanes past their row's
// length only vote "not bad".  (Packing whole rows by their lengths would
// fill the lanes better, but it needs a prefix sum per wave to find the row
// bounds, and the gather is a few microseconds next to K1.)
constexpr int kPtRowLanes = kPathsMaxN + 1;
constexpr int kPtRowsPerWave = 64 / kPtRowLanes;

__global__ __launch_bounds__(kPtThreads) void paths_gather_ragged_kernel(
    const tspgpu_city *__restrict__ cities, const int32_t *__restrict__ tour, int tour_stride,
    const int32_t *__restrict__ status, const BlockDesc *__restrict__ desc, int nblocks,
    tspgpu_city *__restrict__ paths, PathFacts *__restrict__ facts)
{
    __shared__ Seen wseen[kPtWaves];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = lane / kPtRowLanes;      // this lane's row of the wave's group
    const int i = lane - r * kPtRowLanes;  // its city of the row
    const bool mine = r < kPtRowsPerWave;
    const unsigned long long rowmask = mine ? ((1ull << kPtRowLanes) - 1ull) << (r * kPtRowLanes) : 0ull;
    Seen s{~0ull, 0ull, ~0ull, 0ull, INT_MAX, INT_MIN, 0u};
    const long long groups = ((long long)nblocks + kPtRowsPerWave - 1) / kPtRowsPerWave;
    // (the trip count is wave-uniform: every lane reaches the ballot)
    for (long long g = (long long)blockIdx.x * kPtWaves + wave; g < groups; g += (long long)gridDim.x * kPtWaves) {
        const long long b = g * kPtRowsPerWave + r;
        const bool live = mine && b < nblocks;
        int st = 0, n = 0, L = 0;
        long long city = 0, path = 0;
        if (live) {
            const BlockDesc e = desc[b];
            n = e.n, L = e.L, city = e.city, path = e.path;
            if (status) st = status[b];
        }
        if (live && st != 0 && i == 0)
            atomicMin(&facts->first_bad, ((unsigned long long)b << 32) | (unsigned long long)(unsigned)st);
        const bool read = live && st == 0 && i < L;  // (a bad block's tour row is never read)
        const int32_t *row = tour + b * tour_stride;
        int t = 0;
        if (read) t = row[i];
        const bool bad = read && (t < 0 || t >= n);
        const bool rowbad = (__builtin_amdgcn_ballot_w64(bad) & rowmask) != 0ull;
        if (rowbad) s.flags |= kPathBadIndex;
        if (read && !rowbad) {
            const unsigned long long *src = reinterpret_cast<const unsigned long long *>(cities + (city + t));
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(paths + (path + i));
            const unsigned long long w0 = src[0], w1 = src[1], w2 = src[2];
            dst[0] = w0, dst[1] = w1, dst[2] = w2;
            const int id = (int)(unsigned)w0;
            s.id_min = id < s.id_min ? id : s.id_min;
            s.id_max = id > s.id_max ? id : s.id_max;
            if (i == L - 1) {
                // (entry 0 of this row passed the range check above)
                const int id0 = cities[city + row[0]].id;
                if (id != id0) s.flags |= kPathOpen;
            }
            const double x = __builtin_bit_cast(double, w1), y = __builtin_bit_cast(double, w2);
            if (!__builtin_isfinite(x)) {
                s.flags |= kPathNonFinite;
            } else {
                const unsigned long long k = path_order_key(x);
                s.xmin = k < s.xmin ? k : s.xmin;
                s.xmax = k > s.xmax ? k : s.xmax;
            }
            if (!__builtin_isfinite(y)) {
                s.flags |= kPathNonFinite;
            } else {
                const unsigned long long k = path_order_key(y);
                s.ymin = k < s.ymin ? k : s.ymin;
                s.ymax = k > s.ymax ? k : s.ymax;
            }
        }
    }
    seen_publish(s, wseen, lane, wave, facts);
}

// One lane per gathered city with the gather's mapping; a block's last lane
// (its closing copy: the last city of the block's path) sits out.  total: all
// gathered cities, which fits an int (the caller checks).
__global__ __launch_bounds__(kPtThreads) void paths_unique_ragged_kernel(const tspgpu_city *__restrict__ paths,
                                                                        const BlockDesc *__restrict__ desc,
                                                                        int nblocks, unsigned long long total,
                                                                        uint32_t *__restrict__ bitmap,
                                                                        PathFacts *facts)
{
    if (facts->first_bad != ~0ull || (facts->flags & kPathBadIndex)) return;
    const long long lo = facts->id_min, hi = facts->id_max;
    if (hi < lo) return;
    if (!path_ids_fit_bitmap_total(lo, hi, total)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&facts->flags, kPathWideIds);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane / kPtRowLanes, i = lane - r * kPtRowLanes;
    if (r >= kPtRowsPerWave) return;
    const long long groups = ((long long)nblocks + kPtRowsPerWave - 1) / kPtRowsPerWave;
    bool dup = false;
    for (long long g = (long long)blockIdx.x * kPtWaves + wave; g < groups; g += (long long)gridDim.x * kPtWaves) {
        const long long b = g * kPtRowsPerWave + r;
        if (b >= nblocks) continue;
        const BlockDesc e = desc[b];
        if (i >= e.L - 1) continue;  // past the path, or its closing copy
        const long long id = paths[e.path + i].id;
        if (id < lo || id > hi) continue;  // (cannot happen: the extrema are over these ids)
        const unsigned long long bit = (unsigned long long)(id - lo);
        const uint32_t m = 1u << (bit & 31u);
        if (atomicOr(&bitmap[bit >> 5], m) & m) dup = true;
    }
    if (dup) atomicOr(&facts->flags, kPathDupId);
}

// one thread per gathered city (closing copies skipped); nblocks * L fits an
// int (the caller checks), so the index arithmetic is 32-bit
__global__ __launch_bounds__(kPtThreads) void paths_unique_kernel(const tspgpu_city *__restrict__ paths, int L,
                                                                 int nblocks, uint32_t *__restrict__ bitmap,
                                                                 PathFacts *facts)
{
    if (facts->first_bad != ~0ull || (facts->flags & kPathBadIndex)) return;
    const long long lo = facts->id_min, hi = facts->id_max;
    if (hi < lo) return;
    const unsigned long long bits = 8ull * (unsigned long long)nblocks * (unsigned long long)L;
    if ((unsigned long long)(hi - lo) >= bits) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&facts->flags, kPathWideIds);
        return;
    }
    const unsigned total = (unsigned)nblocks * (unsigned)L;
    bool dup = false;
    for (unsigned k = blockIdx.x * kPtThreads + threadIdx.x; k < total; k += gridDim.x * kPtThreads) {
        if (k % (unsigned)L == (unsigned)(L - 1)) continue;  // the closing copy
        const long long id = paths[k].id;
        if (id < lo || id > hi) continue;  // (cannot happen: the extrema are over these ids)
        const unsigned long long bit = (unsigned long long)(id - lo);
        const uint32_t m = 1u << (bit & 31u);
        if (atomicOr(&bitmap[bit >> 5], m) & m) dup = true;
    }
    if (dup) atomicOr(&facts->flags, kPathDupId);
}

int grid_for(unsigned long long workgroups, int grid_cap)
{
    const unsigned long long cap = grid_cap > 0 ? (unsigned long long)grid_cap : 1ull;
    return (int)(workgroups < 1 ? 1 : (workgroups < cap ? workgroups : cap));
}

}  // namespace

hipError_t launch_paths_gather(const tspgpu_city *d_cities, const int32_t *d_tour, const int32_t *d_status, int n,
                               int nblocks, tspgpu_city *d_paths, PathFacts *d_facts, int grid_cap, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (n < 2 || n > kPathsMaxN) return hipErrorInvalidValue;
    int L = tspgpu_tour_length(n);
    int rows_per_wave = 64 / (3 * L);  // >= 1: 3 * 21 = 63
    const unsigned long long groups = ((unsigned long long)nblocks + rows_per_wave - 1) / rows_per_wave;
    void *args[] = {&d_cities, &d_tour, &d_status, &n, &L, &nblocks, &rows_per_wave, &d_paths, &d_facts};
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_gather_kernel),
                           dim3(grid_for((groups + kPtWaves - 1) / kPtWaves, grid_cap)), dim3(kPtThreads), args, 0,
                           stream);
}

hipError_t launch_paths_unique(const tspgpu_city *d_paths, int L, int nblocks, uint32_t *d_bitmap, PathFacts *d_facts,
                               int grid_cap, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (L < 2 || (unsigned long long)nblocks * (unsigned long long)L > (unsigned long long)INT_MAX)
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)nblocks * L;
    void *args[] = {&d_paths, &L, &nblocks, &d_bitmap, &d_facts};
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_unique_kernel),
                           dim3(grid_for((total + kPtThreads - 1) / kPtThreads, grid_cap)), dim3(kPtThreads), args, 0,
                           stream);
}

hipError_t launch_paths_gather_ragged(const tspgpu_city *d_cities, const int32_t *d_tour, int tour_stride,
                                      const int32_t *d_status, const BlockDesc *d_desc, int nblocks,
                                      tspgpu_city *d_paths, PathFacts *d_facts, int grid_cap, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (!d_desc || tour_stride < 2) return hipErrorInvalidValue;
    const unsigned long long groups = ((unsigned long long)nblocks + kPtRowsPerWave - 1) / kPtRowsPerWave;
    void *args[] = {&d_cities, &d_tour, &tour_stride, &d_status, &d_desc, &nblocks, &d_paths, &d_facts};
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_gather_ragged_kernel),
                           dim3(grid_for((groups + kPtWaves - 1) / kPtWaves, grid_cap)), dim3(kPtThreads), args, 0,
                           stream);
}

hipError_t launch_paths_unique_ragged(const tspgpu_city *d_paths, const BlockDesc *d_desc, int nblocks,
                                      unsigned long long total, uint32_t *d_bitmap, PathFacts *d_facts, int grid_cap,
                                      hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (!d_desc || total > (unsigned long long)INT_MAX) return hipErrorInvalidValue;
    const unsigned long long groups = ((unsigned long long)nblocks + kPtRowsPerWave - 1) / kPtRowsPerWave;
    void *args[] = {&d_paths, &d_desc, &nblocks, &total, &d_bitmap, &d_facts};
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_unique_ragged_kernel),
                           dim3(grid_for((groups + kPtWaves - 1) / kPtWaves, grid_cap)), dim3(kPtThreads), args, 0,
                           stream);
}

}  // namespace tspgpu
