// Device distance build (tspgpu_distance_matrix_device): the
// reference's computeDistanceMatrix (assignment2.h:184-200) from city
// coordinates in HBM, bit for bit.  The rules that make it exact are
// dist_exact.h's; this file is the three kernels around them.
//
// Build and finish give one 64-lane wave to a block and four blocks to a
// 256-thread workgroup; a lane owns the pairs lane, lane + 64, lane + 128 of
// the block's n(n-1)/2 (at most 190).  Built without the K1 kernels'
// -fno-honor-nans: a NaN coordinate must stay a NaN distance.
//
// The ragged forms are the same kernels with one difference:
// a wave takes its block's (city offset, matrix offset, n) from the descriptor
// table (block_desc.h) where the uniform form computes b*n, b*n*n and reads n
// from the arguments.  n is uniform within a wave, so every lane still makes
// the same kCtPasses trips and reaches every ballot; the four waves of a
// workgroup may hold blocks of four different sizes.
#include "cities.h"

#include "dist_exact.h"
#include "wave.h"

namespace tspgpu {
namespace {

constexpr int kCtThreads = 256;
constexpr int kCtWaves = kCtThreads / 64;
constexpr int kCtPasses = (kCitiesMaxN * (kCitiesMaxN - 1) / 2 + 63) / 64;  // 3: a block's pairs per lane
constexpr int kCtPatchMaxGrid = 1 << 16;  // workgroups; longer lists loop

// pair k (0 <= k < n(n-1)/2, row-major over i < j) -> (i, j)
__device__ __forceinline__ void pair_of(int k, int n, int *i, int *j)
{
    int row = 0, len = n - 1;
    while (k >= len) {
        k -= len;
        ++row;
        --len;
    }
    *i = row;
    *j = row + 1 + k;
}

// lanes below this one among the set bits of a ballot
__device__ __forceinline__ int lanes_below(uint64_t ballot)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// Build: for every pair i < j the reference's operands of entry (i, j),
// dx = x_i - x_j and dy = y_i - y_j (entry (j, i) has the negations, and
// pow(-x, 2) == pow(x, 2)); dx*dx provisionally at d[i][j], dy*dy at d[j][i];
// every flagged square's (slot, operand) appended to the fix-up list with one
// atomic add per wave.  The diagonal is final here: +0.0, or NaN where a
// coordinate is not finite (x - x is NaN then, as in the reference).
// Where block b lies: computed (uniform) or read from the table (ragged; the
// whole wave reads one entry, n made a scalar).
template <bool kRagged>
__device__ __forceinline__ void block_place(const BlockDesc *__restrict__ desc, int64_t b, bool live, int &n,
                                            int64_t &city, int64_t &base)
{
    if constexpr (kRagged) {
        n = 0, city = 0, base = 0;
        if (live) {
            const BlockDesc e = desc[b];
            n = e.n, city = e.city, base = e.dist;
            if (n < 0 || n > kCitiesMaxN) n = 0;  // (the fronts refuse such a table: the LDS rows hold kCitiesMaxN)
        }
        n = __builtin_amdgcn_readfirstlane(n);
    } else {
        city = b * n;
        base = b * n * n;
    }
}

template <bool kRagged>
__global__ __launch_bounds__(kCtThreads) void cities_build_kernel(const tspgpu_city *__restrict__ cities, int n,
                                                                 const BlockDesc *__restrict__ desc, int nblocks,
                                                                 double *__restrict__ dist,
                                                                 int64_t *__restrict__ fix_slot,
                                                                 double *__restrict__ fix_dx,
                                                                 unsigned long long fix_cap,
                                                                 unsigned long long *__restrict__ fix_count)
{
    __shared__ double sx[kCtWaves][kCitiesMaxN], sy[kCtWaves][kCitiesMaxN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t b = (int64_t)blockIdx.x * kCtWaves + wave;
    const bool live = b < nblocks;
    int64_t city, base;
    block_place<kRagged>(desc, b, live, n, city, base);
    if (live && lane < n) {
        const tspgpu_city c = cities[city + lane];
        sx[wave][lane] = c.x;
        sy[wave][lane] = c.y;
    }
    __syncthreads();
    if (!live) return;
    const int pairs = n * (n - 1) / 2;
    double *d = dist + base;
    if (lane < n) {
        const double zx = sx[wave][lane] - sx[wave][lane], zy = sy[wave][lane] - sy[wave][lane];
        d[lane * n + lane] = (zx == 0.0 && zy == 0.0) ? 0.0 : zx * zx + zy * zy;
    }
    double opx[kCtPasses], opy[kCtPasses];
    int slx[kCtPasses], sly[kCtPasses];
    bool fx[kCtPasses], fy[kCtPasses];
    uint64_t bx[kCtPasses], by[kCtPasses];
    int total = 0;
#pragma unroll
    for (int p = 0; p < kCtPasses; ++p) {
        const int k = lane + 64 * p;
        fx[p] = fy[p] = false;
        opx[p] = opy[p] = 0.0;
        slx[p] = sly[p] = 0;
        if (k < pairs) {
            int i, j;
            pair_of(k, n, &i, &j);
            opx[p] = sx[wave][i] - sx[wave][j];
            opy[p] = sy[wave][i] - sy[wave][j];
            double px, py;
            fx[p] = square_needs_host(opx[p], &px);
            fy[p] = square_needs_host(opy[p], &py);
            slx[p] = i * n + j;
            sly[p] = j * n + i;
            d[slx[p]] = px;
            d[sly[p]] = py;
        }
        bx[p] = __builtin_amdgcn_ballot_w64(fx[p]);
        by[p] = __builtin_amdgcn_ballot_w64(fy[p]);
        total += __builtin_popcountll(bx[p]) + __builtin_popcountll(by[p]);
    }
    if (total == 0) return;  // (wave-uniform)
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(fix_count, (unsigned long long)total);
    at = wave_detail::readlane64(at, 0);
#pragma unroll
    for (int p = 0; p < kCtPasses; ++p) {
        if (fx[p]) {
            const unsigned long long t = at + (unsigned)lanes_below(bx[p]);
            if (t < fix_cap) {
                fix_slot[t] = base + slx[p];
                fix_dx[t] = opx[p];
            }
        }
        at += (unsigned)__builtin_popcountll(bx[p]);
        if (fy[p]) {
            const unsigned long long t = at + (unsigned)lanes_below(by[p]);
            if (t < fix_cap) {
                fix_slot[t] = base + sly[p];
                fix_dx[t] = opy[p];
            }
        }
        at += (unsigned)__builtin_popcountll(by[p]);
    }
}

__global__ __launch_bounds__(kCtThreads) void cities_patch_kernel(double *__restrict__ dist,
                                                                 const int64_t *__restrict__ fix_slot,
                                                                 const double *__restrict__ fix_val,
                                                                 unsigned long long count)
{
    for (unsigned long long t = (unsigned long long)blockIdx.x * kCtThreads + threadIdx.x; t < count;
         t += (unsigned long long)gridDim.x * kCtThreads)
        dist[fix_slot[t]] = fix_val[t];
}

// Finish: the two squares of a pair sit at d[i][j] and d[j][i]; both entries
// become sqrt_rn of their sum (the lane that owns the pair is the only one
// that touches either).
template <bool kRagged>
__global__ __launch_bounds__(kCtThreads) void cities_finish_kernel(int n, const BlockDesc *__restrict__ desc,
                                                                  int nblocks, double *__restrict__ dist)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t b = (int64_t)blockIdx.x * kCtWaves + wave;
    if (b >= nblocks) return;
    int64_t city, base;
    block_place<kRagged>(desc, b, true, n, city, base);
    const int pairs = n * (n - 1) / 2;
    double *d = dist + base;
#pragma unroll
    for (int p = 0; p < kCtPasses; ++p) {
        const int k = lane + 64 * p;
        if (k < pairs) {
            int i, j;
            pair_of(k, n, &i, &j);
            const double s = sqrt_rn(d[i * n + j] + d[j * n + i]);
            d[i * n + j] = s;
            d[j * n + i] = s;
        }
    }
}

unsigned ct_grid(int nblocks) { return (unsigned)(((int64_t)nblocks + kCtWaves - 1) / kCtWaves); }

}  // namespace

hipError_t launch_cities_build(const tspgpu_city *cities, int n, int nblocks, double *dist, int64_t *fix_slot,
                               double *fix_dx, unsigned long long fix_cap, unsigned long long *fix_count,
                               hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (n < 1 || n > kCitiesMaxN) return hipErrorInvalidValue;
    const BlockDesc *desc = nullptr;
    void *args[] = {&cities, &n, &desc, &nblocks, &dist, &fix_slot, &fix_dx, &fix_cap, &fix_count};
    return hipLaunchKernel(reinterpret_cast<const void *>(&cities_build_kernel<false>), dim3(ct_grid(nblocks)),
                           dim3(kCtThreads), args, 0, stream);
}

hipError_t launch_cities_build_ragged(const tspgpu_city *cities, const BlockDesc *desc, int nblocks, double *dist,
                                      int64_t *fix_slot, double *fix_dx, unsigned long long fix_cap,
                                      unsigned long long *fix_count, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (!desc) return hipErrorInvalidValue;
    int n = 0;
    void *args[] = {&cities, &n, &desc, &nblocks, &dist, &fix_slot, &fix_dx, &fix_cap, &fix_count};
    return hipLaunchKernel(reinterpret_cast<const void *>(&cities_build_kernel<true>), dim3(ct_grid(nblocks)),
                           dim3(kCtThreads), args, 0, stream);
}

hipError_t launch_cities_patch(double *dist, const int64_t *fix_slot, const double *fix_val,
                               unsigned long long count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    const unsigned long long wg = (count + kCtThreads - 1) / kCtThreads;
    void *args[] = {&dist, &fix_slot, &fix_val, &count};
    return hipLaunchKernel(reinterpret_cast<const void *>(&cities_patch_kernel),
                           dim3((unsigned)(wg < (unsigned long long)kCtPatchMaxGrid ? wg : kCtPatchMaxGrid)),
                           dim3(kCtThreads), args, 0, stream);
}

hipError_t launch_cities_finish(int n, int nblocks, double *dist, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (n < 1 || n > kCitiesMaxN) return hipErrorInvalidValue;
    const BlockDesc *desc = nullptr;
    void *args[] = {&n, &desc, &nblocks, &dist};
    return hipLaunchKernel(reinterpret_cast<const void *>(&cities_finish_kernel<false>), dim3(ct_grid(nblocks)),
                           dim3(kCtThreads), args, 0, stream);
}

hipError_t launch_cities_finish_ragged(const BlockDesc *desc, int nblocks, double *dist, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (!desc) return hipErrorInvalidValue;
    int n = 0;
    void *args[] = {&n, &desc, &nblocks, &dist};
    return hipLaunchKernel(reinterpret_cast<const void *>(&cities_finish_kernel<true>), dim3(ct_grid(nblocks)),
                           dim3(kCtThreads), args, 0, stream);
}

}  // namespace tspgpu
