// Ragged K1 batches (tspgpu_solve_ragged*): one pass over the
// caller's matrices that validates every block and gathers it into its size
// bucket, and one pass that puts the buckets' answers back in caller order.
//
// Both kernels give one 64-lane wave to a block, four blocks to a 256-thread
// workgroup, with no barrier and no state shared between waves: a wave whose
// block index is past the batch leaves.  Built without the K1 kernels'
// -fno-honor-nans: the validation is done on the values' bits anyway.
#include "ragged.h"

#include <cerrno>
#include <climits>

#include "wave.h"

namespace tspgpu {
namespace {

constexpr int kRgThreads = 256;
constexpr int kRgWaves = kRgThreads / 64;
constexpr int kRgPasses = (kRaggedMaxN * kRaggedMaxN + 63) / 64;  // 7: a block's elements per lane
constexpr int kRgMaxGrid = 1 << 20;  // workgroups; larger batches loop

// Bit-level view of a value type: the unsigned carrier whose order is the
// values' order on every valid (non-negative, finite) value, and the
// predicate of tspgpu_validate / tspgpu_validate_i32.
template <typename V> struct RgVal;
template <> struct RgVal<double> {
    using U = uint64_t;
    __device__ static U bits(double v) { return (U)__double_as_longlong(v); }
    // negative (and -0.0, -inf, NaN with the sign set): sign bit; +inf, NaN: exponent all ones
    __device__ static bool bad(U u) { return (u >> 63) != 0 || ((u >> 52) & 0x7ffu) == 0x7ffu; }
    __device__ static bool over(int n, U mx) { return (double)n * __longlong_as_double((long long)mx) >= (double)INT_MAX; }
    __device__ static double refused() { return __longlong_as_double(0x7ff8000000000000ll); }  // NaN
};
template <> struct RgVal<int32_t> {
    using U = uint32_t;
    __device__ static U bits(int32_t v) { return (U)v; }
    __device__ static bool bad(U u) { return (u >> 31) != 0; }
    __device__ static bool over(int n, U mx) { return (int64_t)n * (int64_t)mx >= (int64_t)INT_MAX; }
    __device__ static int32_t refused() { return -1; }
};

__device__ __forceinline__ uint64_t umax(uint64_t a, uint64_t b) { return a < b ? b : a; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a < b ? b : a; }

template <int CTRL> __device__ __forceinline__ uint64_t rg_dpp(uint64_t v) { return wave_detail::dpp64<CTRL>(v); }
template <int CTRL> __device__ __forceinline__ uint32_t rg_dpp(uint32_t v) { return wave_detail::dpp32<CTRL>(v); }
__device__ __forceinline__ uint64_t rg_readlane(uint64_t v, int lane) { return wave_detail::readlane64(v, lane); }
__device__ __forceinline__ uint32_t rg_readlane(uint32_t v, int lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// maximum over the 64 lanes (every lane active), wave-uniform: wave_min_dpp's
// steps (wave.h) on an unsigned carrier
template <typename U>
__device__ __forceinline__ U wave_max_dpp(U v)
{
    using namespace wave_detail;
    v = umax(v, rg_dpp<kDppXor1>(v));
    v = umax(v, rg_dpp<kDppXor2>(v));
    v = umax(v, rg_dpp<kDppHalfMirror>(v));
    v = umax(v, rg_dpp<kDppMirror>(v));
    return umax(umax(rg_readlane(v, 0), rg_readlane(v, 16)), umax(rg_readlane(v, 32), rg_readlane(v, 48)));
}

// Gather: block b's n*n elements from src + desc[b].src (element aligned only;
// sources may overlap, repeat and come in any order) to its bucket slot
// stage + desc[b].dst.  One read pass into registers, the wave-wide verdict,
// one write pass: the elements of a valid block, zeros for any other (an
// all-tie matrix K1 solves like any; the scatter drops its answer).
template <typename V>
__global__ __launch_bounds__(kRgThreads) void ragged_gather_kernel(const V *__restrict__ src,
                                                                  const RaggedDesc *__restrict__ desc, int nblocks,
                                                                  V *__restrict__ stage,
                                                                  int32_t *__restrict__ stage_status)
{
    using R = RgVal<V>;
    using U = typename R::U;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t b = (int64_t)blockIdx.x * kRgWaves + wave; b < nblocks; b += (int64_t)gridDim.x * kRgWaves) {
        const RaggedDesc e = desc[b];
        if (e.pre != 0) {  // refused by the plan: in no bucket, never read
            if (lane == 0) stage_status[b] = e.pre;
            continue;
        }
        const int n = e.n, nn = n * n;
        const V *s = src + e.src;
        U u[kRgPasses];
#pragma unroll
        for (int p = 0; p < kRgPasses; ++p) {
            const int i = lane + 64 * p;
            u[p] = i < nn ? R::bits(s[i]) : U(0);
        }
        bool bad = false;
        U mx = 0;
#pragma unroll
        for (int p = 0; p < kRgPasses; ++p) {
            bad |= R::bad(u[p]);
            mx = umax(mx, u[p]);
        }
        // the flag by ballot, apart from the maximum (a bad element's bits are
        // above every valid value's; the maximum only matters without one)
        const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
        mx = wave_max_dpp(mx);
        const int st = any_bad ? -EINVAL : (R::over(n, mx) ? -ERANGE : 0);
        V *d = stage + e.dst;
#pragma unroll
        for (int p = 0; p < kRgPasses; ++p) {
            const int i = lane + 64 * p;
            if (i < nn) {
                const U out = st == 0 ? u[p] : U(0);
                reinterpret_cast<U *>(d)[i] = out;
            }
        }
        if (lane == 0) stage_status[b] = st;
    }
}

// Scatter: block b's cost and tour from its bucket back to row b.  K1 writes
// tspgpu_tour_length(n) tour entries (two at n = 2), so no more are copied;
// the rest of the row is -1.
template <typename V>
__global__ __launch_bounds__(kRgThreads) void ragged_scatter_kernel(
    const RaggedDesc *__restrict__ desc, const int32_t *__restrict__ stage_status, int nblocks,
    const V *__restrict__ stage_cost, const int32_t *__restrict__ stage_tour, V *__restrict__ cost_out,
    int32_t *__restrict__ tour_out, int tour_stride, int32_t *__restrict__ status_out)
{
    using R = RgVal<V>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t b = (int64_t)blockIdx.x * kRgWaves + wave; b < nblocks; b += (int64_t)gridDim.x * kRgWaves) {
        const RaggedDesc e = desc[b];
        int st = stage_status[b];
        V c = R::refused();
        if (st == 0) {
            c = stage_cost[e.cost];
            if (c < V(0)) {  // K1's backtracking found no predecessor
                st = -EIO;
                c = R::refused();
            }
        }
        const int len = e.n == 2 ? 2 : e.n + 1;  // tspgpu_tour_length
        const int32_t *t = stage_tour + e.tour;
        int32_t *row = tour_out + b * (int64_t)tour_stride;
        for (int j = lane; j < tour_stride; j += 64) row[j] = st == 0 && j < len ? t[j] : -1;
        if (lane == 0) {
            cost_out[b] = c;
            status_out[b] = st;
        }
    }
}

int rg_grid(int nblocks)
{
    const int64_t wg = ((int64_t)nblocks + kRgWaves - 1) / kRgWaves;
    return (int)(wg < kRgMaxGrid ? wg : kRgMaxGrid);
}

template <typename V>
hipError_t gather_v(const void *src, const RaggedDesc *desc, int nblocks, void *stage, int32_t *stage_status,
                    hipStream_t stream)
{
    const V *s = static_cast<const V *>(src);
    V *d = static_cast<V *>(stage);
    void *args[] = {&s, &desc, &nblocks, &d, &stage_status};
    return hipLaunchKernel(reinterpret_cast<const void *>(&ragged_gather_kernel<V>), dim3(rg_grid(nblocks)),
                           dim3(kRgThreads), args, 0, stream);
}

template <typename V>
hipError_t scatter_v(const RaggedDesc *desc, const int32_t *stage_status, int nblocks, const void *stage_cost,
                     const int32_t *stage_tour, void *cost_out, int32_t *tour_out, int tour_stride,
                     int32_t *status_out, hipStream_t stream)
{
    const V *sc = static_cast<const V *>(stage_cost);
    V *co = static_cast<V *>(cost_out);
    void *args[] = {&desc, &stage_status, &nblocks, &sc, &stage_tour, &co, &tour_out, &tour_stride, &status_out};
    return hipLaunchKernel(reinterpret_cast<const void *>(&ragged_scatter_kernel<V>), dim3(rg_grid(nblocks)),
                           dim3(kRgThreads), args, 0, stream);
}

}  // namespace

hipError_t launch_ragged_gather(int vbytes, const void *src, const RaggedDesc *desc, int nblocks, void *stage_dist,
                                int32_t *stage_status, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (vbytes == 8) return gather_v<double>(src, desc, nblocks, stage_dist, stage_status, stream);
    if (vbytes == 4) return gather_v<int32_t>(src, desc, nblocks, stage_dist, stage_status, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_ragged_scatter(int vbytes, const RaggedDesc *desc, const int32_t *stage_status, int nblocks,
                                 const void *stage_cost, const int32_t *stage_tour, void *cost_out,
                                 int32_t *tour_out, int tour_stride, int32_t *status_out, hipStream_t stream)
{
    if (nblocks <= 0) return hipSuccess;
    if (vbytes == 8)
        return scatter_v<double>(desc, stage_status, nblocks, stage_cost, stage_tour, cost_out, tour_out, tour_stride,
                                 status_out, stream);
    if (vbytes == 4)
        return scatter_v<int32_t>(desc, stage_status, nblocks, stage_cost, stage_tour, cost_out, tour_out,
                                  tour_stride, status_out, stream);
    return hipErrorInvalidValue;
}

}  // namespace tspgpu
