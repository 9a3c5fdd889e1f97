// Fixed-end paths and the window refinement (tspgpu_solve_paths*,
// tspgpu_refine_path*): the kernels around K1.  fold turns the
// w x w matrices into the (w-1) x (w-1) ones K1 solves; gather copies a
// pass's windows out of the path; apply splices the strictly better orders
// back.  All memory-bound: 8-byte accesses along consecutive lanes, 64-bit
// element offsets (W * w * w elements pass 2^31 near 10^7 cities).  Built
// without the K1 kernels' -fno-honor-nans: a refused window's NaN cost must
// compare false.
#include "refine.h"

namespace tspgpu {
namespace {

constexpr int kRfThreads = 256;
constexpr int kRfWaves = kRfThreads / 64;
constexpr int kRfMaxGrid = 1 << 20;  // workgroups; larger batches loop
constexpr int kCityWords = 3;        // a city as 8-byte words: id + padding, x, y
static_assert(sizeof(tspgpu_city) == kCityWords * sizeof(uint64_t), "a city is three 8-byte words");

int rf_grid(int64_t items, int per_group)
{
    const int64_t wg = (items + per_group - 1) / per_group;
    return (int)(wg < 1 ? 1 : (wg < kRfMaxGrid ? wg : kRfMaxGrid));
}

// One output element per lane, consecutive lanes on consecutive elements.  The
// 64-bit division is taken once per workgroup pass (on its first element);
// the lanes divide small 32-bit numbers.
template <typename V>
__global__ __launch_bounds__(kRfThreads) void paths_fold_kernel(const V *__restrict__ dist, int w, int64_t nblocks,
                                                               V *__restrict__ fold)
{
    const int n = w - 1, nn = n * n, ww = w * w;
    const int64_t total = nblocks * nn;
    for (int64_t base = (int64_t)blockIdx.x * kRfThreads; base < total; base += (int64_t)gridDim.x * kRfThreads) {
        const int64_t b0 = base / nn;
        const int local = (int)(base - b0 * nn) + (int)threadIdx.x;
        const int db = local / nn, r = local - db * nn;
        const int64_t b = b0 + db;
        if (b >= nblocks) continue;
        const int i = r / n, j = r - i * n;
        const V *d = dist + b * ww;
        V v = V(0);  // P[0][0]
        if (j >= 1)
            v = d[i * w + j];
        else if (i >= 1)
            v = d[i * w + n];  // the way to the fixed end, D[i][w-1]
        fold[b * nn + r] = v;
    }
}

__global__ __launch_bounds__(kRfThreads) void paths_identity_cost_kernel(const double *__restrict__ dist, int w,
                                                                        int64_t nblocks,
                                                                        double *__restrict__ old_cost)
{
    const int ww = w * w;
    for (int64_t b = (int64_t)blockIdx.x * kRfThreads + threadIdx.x; b < nblocks;
         b += (int64_t)gridDim.x * kRfThreads) {
        const double *d = dist + b * ww;
        double s = d[1];
        for (int i = 1; i < w - 1; ++i) s = s + d[i * w + i + 1];
        old_cost[b] = s;
    }
}

__global__ __launch_bounds__(kRfThreads) void paths_close_kernel(int32_t *__restrict__ order,
                                                                const int32_t *__restrict__ status, int w,
                                                                int64_t nblocks)
{
    for (int64_t b = (int64_t)blockIdx.x * kRfThreads + threadIdx.x; b < nblocks;
         b += (int64_t)gridDim.x * kRfThreads)
        if (status[b] == 0) order[b * w + (w - 1)] = w - 1;
}

// One 8-byte word per lane: the packed copy is written in order, window k's
// 3w words read from the path at (offset + k * stride) cities.
__global__ __launch_bounds__(kRfThreads) void refine_gather_kernel(const uint64_t *__restrict__ path, int64_t offset,
                                                                  int64_t stride, int w, int64_t windows,
                                                                  uint64_t *__restrict__ packed)
{
    const int per = kCityWords * w;
    const int64_t total = windows * per;
    for (int64_t base = (int64_t)blockIdx.x * kRfThreads; base < total; base += (int64_t)gridDim.x * kRfThreads) {
        const int64_t k0 = base / per;
        const int local = (int)(base - k0 * per) + (int)threadIdx.x;
        const int dk = local / per, r = local - dk * per;
        const int64_t k = k0 + dk;
        if (k >= windows) continue;
        packed[k * per + r] = path[(offset + k * stride) * kCityWords + r];
    }
}

// One wave per window, one lane per 8-byte word of its interior (3m <= 54).
// Every word comes from the packed copy of the pass, so no lane reads a
// position any window writes; neighbours share only their fixed ends, which
// nobody writes.
__global__ __launch_bounds__(kRfThreads) void refine_apply_kernel(
    uint64_t *__restrict__ path, int64_t offset, int64_t stride, int w, int64_t windows,
    const uint64_t *__restrict__ packed, const int32_t *__restrict__ tour, const int32_t *__restrict__ status,
    const double *__restrict__ cost, const double *__restrict__ old_cost, double *__restrict__ gain,
    int32_t *__restrict__ replaced)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = w - 2;
    for (int64_t k = (int64_t)blockIdx.x * kRfWaves + wave; k < windows; k += (int64_t)gridDim.x * kRfWaves) {
        const double nw = cost[k], od = old_cost[k];
        bool take = status[k] == 0 && nw < od;  // strictly better; a tie keeps the old order
        const int j = 1 + lane / kCityWords, word = lane - (j - 1) * kCityWords;
        const bool mine = lane < kCityWords * m;
        int t = 1;
        if (take && mine) t = tour[k * w + j];
        // (K1's rows are permutations of 1..m under status 0; an entry outside
        // would index outside the window: such a window is left as it is)
        const bool bad = t < 1 || t > m;
        take = take && __builtin_amdgcn_ballot_w64(bad) == 0;
        if (take && mine)
            path[(offset + k * stride + j) * kCityWords + word] = packed[(k * w + t) * kCityWords + word];
        if (lane == 0) {
            gain[k] = take ? od - nw : 0.0;
            replaced[k] = take ? 1 : 0;
        }
    }
}

template <typename V>
hipError_t fold_v(const void *dist, int w, int64_t nblocks, void *fold, hipStream_t stream)
{
    const V *s = static_cast<const V *>(dist);
    V *d = static_cast<V *>(fold);
    void *args[] = {&s, &w, &nblocks, &d};
    const int64_t total = nblocks * (w - 1) * (w - 1);
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_fold_kernel<V>), dim3(rf_grid(total, kRfThreads)),
                           dim3(kRfThreads), args, 0, stream);
}

}  // namespace

hipError_t launch_paths_fold(int vbytes, const void *dist, int w, int64_t nblocks, void *fold, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (w < 3) return hipErrorInvalidValue;
    if (vbytes == 8) return fold_v<double>(dist, w, nblocks, fold, stream);
    if (vbytes == 4) return fold_v<int32_t>(dist, w, nblocks, fold, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_paths_identity_cost(const double *dist, int w, int64_t nblocks, double *old_cost,
                                      hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (w < 3) return hipErrorInvalidValue;
    void *args[] = {&dist, &w, &nblocks, &old_cost};
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_identity_cost_kernel),
                           dim3(rf_grid(nblocks, kRfThreads)), dim3(kRfThreads), args, 0, stream);
}

hipError_t launch_paths_close(int32_t *order, const int32_t *status, int w, int64_t nblocks, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    void *args[] = {&order, &status, &w, &nblocks};
    return hipLaunchKernel(reinterpret_cast<const void *>(&paths_close_kernel), dim3(rf_grid(nblocks, kRfThreads)),
                           dim3(kRfThreads), args, 0, stream);
}

hipError_t launch_refine_gather(const tspgpu_city *path, int64_t offset, int64_t stride, int w, int64_t windows,
                                tspgpu_city *packed, hipStream_t stream)
{
    if (windows <= 0) return hipSuccess;
    const uint64_t *s = reinterpret_cast<const uint64_t *>(path);
    uint64_t *d = reinterpret_cast<uint64_t *>(packed);
    void *args[] = {&s, &offset, &stride, &w, &windows, &d};
    return hipLaunchKernel(reinterpret_cast<const void *>(&refine_gather_kernel),
                           dim3(rf_grid(windows * kCityWords * w, kRfThreads)), dim3(kRfThreads), args, 0, stream);
}

hipError_t launch_refine_apply(tspgpu_city *path, int64_t offset, int64_t stride, int w, int64_t windows,
                               const tspgpu_city *packed, const int32_t *tour, const int32_t *status,
                               const double *cost, const double *old_cost, double *gain, int32_t *replaced,
                               hipStream_t stream)
{
    if (windows <= 0) return hipSuccess;
    if (w < 4 || kCityWords * (w - 2) > 64) return hipErrorInvalidValue;
    uint64_t *p = reinterpret_cast<uint64_t *>(path);
    const uint64_t *s = reinterpret_cast<const uint64_t *>(packed);
    void *args[] = {&p, &offset, &stride, &w, &windows, &s, &tour, &status, &cost, &old_cost, &gain, &replaced};
    return hipLaunchKernel(reinterpret_cast<const void *>(&refine_apply_kernel), dim3(rf_grid(windows, kRfWaves)),
                           dim3(kRfThreads), args, 0, stream);
}

}  // namespace tspgpu
