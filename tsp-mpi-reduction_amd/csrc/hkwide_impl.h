// K1-wide — ONE instance's Held-Karp over the whole GPU (all CUs cooperate
// on every layer), for the single-instance time to the optimal tour and for
// instances past K1's per-workgroup sizes (n <= 31: the table of
// N*2^(N-1) values is 129 GB of doubles / 65 GB of int32 at n = 31 and fits
// one MI355X's 288 GB).
//
// Same recurrence and the same IEEE operations as K1 / tsp.cpp:405-509, so the
// same bits: layer s is computed from layer s-1 by one launch with a thread
// per DESTINATION state (S, k) in the position-major layout of K1
// (heldkarp_impl.h): element e = p*C(N,s) + colexrank(S), p = position of k
// in S, so the writes of a wave are one contiguous segment.  The thread
// unranks S from colexrank(S) (binomials in LDS, no 2^N mask table), drops
// k, and takes the first-strict-min-free min over the members m of T = S\k of
// G[T][m] + d[m][k] (the min itself is order independent; the tie-break
// happens in the backtracking, which picks the smallest m whose candidate
// equals the state value, as K1 does).  A one-wave kernel closes the tour
// (tsp.cpp:483-499) and backtracks.
//
// Everything here is generic over the value type V: double (hkwide.hip, the
// reference's distances) or int32_t (hkwide_i32.hip, the integer-weight
// extension: integer add and min, INT_MAX sentinel, a table of half the
// bytes).  Each translation unit instantiates one V, so each code object
// holds one set of kernels.  Offsets and counts are in elements.
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "ctx.h"
#include "xfer.h"
#include "wave.h"
#include "tspgpu.h"
#include "tuning.h"

namespace tspgpu_wide {

using tspgpu::xcopy_async;

constexpr int kWideMaxN = 30;  // inner cities (n <= 31: a 129 GB f64 table)
constexpr int kWideThreads = 256;

// What differs between the value types: the sentinel every min starts from
// (tsp.cpp:453; candidates are below it by validation), what an invalid lane
// of the closing wave carries, the min itself, and the failure mark.
template <typename V> struct WideVal;
template <> struct WideVal<double> {
    static constexpr int dtype = TSPGPU_F64;
    static constexpr double sentinel = 2147483647.0;
    static constexpr double invalid = 1.0e300;
    static constexpr double failed = -1.0;
    __device__ static __forceinline__ double vmin(double a, double b) { return fmin(a, b); }
};
template <> struct WideVal<int32_t> {
    static constexpr int dtype = TSPGPU_I32;
    static constexpr int32_t sentinel = INT_MAX;
    static constexpr int32_t invalid = INT_MAX;
    static constexpr int32_t failed = -1;
    __device__ static __forceinline__ int32_t vmin(int32_t a, int32_t b) { return b < a ? b : a; }
};

struct WideInfo {
    long long binom[kWideMaxN + 2][kWideMaxN + 2];  // C(a, b)
    unsigned long long off[kWideMaxN + 2];          // elements before layer t
    unsigned long long cnt[kWideMaxN + 2];          // C(N, t)
};

__device__ __forceinline__ long long bn(const long long (*b)[kWideMaxN + 2], int a, int k)
{
    return (k < 0 || k > a) ? 0 : b[a][k];
}

// layer 1: G[{i}][i] = d[0][i+1]
template <typename V>
__global__ void wide_layer1(const V *__restrict__ d, int n, V *__restrict__ tab)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n - 1) tab[i] = d[i + 1];
}

template <typename V>
__global__ __launch_bounds__(kWideThreads) void wide_layer(const V *__restrict__ dist, int N,
                                                           const WideInfo *__restrict__ info, int s,
                                                           V *__restrict__ tab)
{
    __shared__ long long B[kWideMaxN + 2][kWideMaxN + 2];
    __shared__ V dl[(kWideMaxN + 1) * (kWideMaxN + 1)];
    const int n = N + 1;
    for (int i = threadIdx.x; i < (kWideMaxN + 2) * (kWideMaxN + 2); i += kWideThreads)
        (&B[0][0])[i] = (&info->binom[0][0])[i];
    for (int i = threadIdx.x; i < n * n; i += kWideThreads) dl[i] = dist[i];
    __syncthreads();
    const int t = s - 1;
    const unsigned long long cs = info->cnt[s], ct = info->cnt[t];
    const unsigned long long os = info->off[s], ot = info->off[t];
    const unsigned long long total = cs * (unsigned long long)s;
    for (unsigned long long e = blockIdx.x * (unsigned long long)kWideThreads + threadIdx.x; e < total;
         e += (unsigned long long)gridDim.x * kWideThreads) {
        const int p = (int)(e / cs);
        long long r = (long long)(e - (unsigned long long)p * cs);
        // colex unrank: members e_1 < ... < e_s with r = sum C(e_i, i)
        uint32_t S = 0;
        int c = N - 1;
        for (int i = s; i >= 1; --i) {
            while (bn(B, c, i) > r) --c;
            r -= bn(B, c, i);
            S |= 1u << c;
            --c;
        }
        // k = p-th member (ascending); T = S \ k and its colex rank
        uint32_t x = S;
        for (int q = 0; q < p; ++q) x &= x - 1u;
        const int k = __builtin_ctz(x);
        const uint32_t T = S & ~(1u << k);
        long long rT = 0;
        {
            uint32_t y = T;
            int i = 1;
            while (y) {
                const int b = __builtin_ctz(y);
                rT += bn(B, b, i++);
                y &= y - 1u;
            }
        }
        V acc = WideVal<V>::sentinel;  // tsp.cpp:453 (candidates are < INT_MAX by validation)
        uint32_t y = T;
        int j = 0;
        while (y) {
            const int m = __builtin_ctz(y);
            y &= y - 1u;
            const V g = tab[ot + (unsigned long long)j * ct + (unsigned long long)rT];
            acc = WideVal<V>::vmin(acc, g + dl[(m + 1) * n + (k + 1)]);
            ++j;
        }
        tab[os + e] = acc;
    }
}

// Row-owner ("push") form of a layer, t -> t+1 (default): a thread owns a
// SOURCE row T of layer t (its t values are coalesced loads: consecutive
// threads hold consecutive colex ranks) and writes every destination
// G[T+k][k] = min_{m in T} G[T][m] + d[m][k] for the N - t cities k not in T —
// the whole min of a destination comes from that one row, so every table
// entry is read once and written once (the pull form above reads each entry
// N - t times through scattered loads).  The destination rank follows from
// prefix sums over T's members: colexrank(T+k) = sum_{m<k} C(m, i_m) +
// C(k, c+1) + sum_{m>k} C(m, i_m + 1), c = #members below k = the position of
// k in T+k.  Consecutive rows differ in their low members, so the writes of
// one k are mostly contiguous runs.  Templated on t: the row lives in VGPRs.
template <typename V, int T>
__global__ __launch_bounds__(kWideThreads) void wide_push(const V *__restrict__ dist, int N,
                                                          const WideInfo *__restrict__ info,
                                                          V *__restrict__ tab)
{
    __shared__ int B[kWideMaxN + 2][kWideMaxN + 3];  // C(a, b), b <= 31 (ranks < 2^31 for N <= 30)
    __shared__ V dl[(kWideMaxN + 1) * (kWideMaxN + 1)];
    const int n = N + 1;
    for (int i = threadIdx.x; i < (kWideMaxN + 2) * (kWideMaxN + 3); i += kWideThreads) {
        const int a = i / (kWideMaxN + 3), b = i % (kWideMaxN + 3);
        (&B[0][0])[i] = b <= kWideMaxN + 1 ? (int)info->binom[a][b] : 0;
    }
    for (int i = threadIdx.x; i < n * n; i += kWideThreads) dl[i] = dist[i];
    __syncthreads();
    const unsigned long long ct = info->cnt[T], cs = info->cnt[T + 1];
    const unsigned long long ot = info->off[T], os = info->off[T + 1];
    for (unsigned long long r0 = blockIdx.x * (unsigned long long)kWideThreads + threadIdx.x; r0 < ct;
         r0 += (unsigned long long)gridDim.x * kWideThreads) {
        // colex unrank of T: members m_1 < ... < m_T with r0 = sum C(m_i, i)
        int m[T];
        long long r = (long long)r0;
        int c = N - 1;
#pragma unroll
        for (int i = T; i >= 1; --i) {
            while (B[c][i] > r) --c;
            r -= B[c][i];
            m[i - 1] = c;
            --c;
        }
        V g[T];
#pragma unroll
        for (int j = 0; j < T; ++j) g[j] = tab[ot + (unsigned long long)j * ct + r0];
        uint32_t mask = 0;
        long long hi = 0;  // sum_j C(m_j, j+2): every member above k
#pragma unroll
        for (int j = 0; j < T; ++j) {
            mask |= 1u << m[j];
            hi += B[m[j]][j + 2];
        }
        long long lo = 0;  // sum over members below k of C(m_j, j+1) - C(m_j, j+2)
        int cb = 0;        // members below k
        for (int k = 0; k < N; ++k) {
            if ((mask >> k) & 1u) {
                lo += (long long)B[k][cb + 1] - (long long)B[k][cb + 2];
                ++cb;
                continue;
            }
            V acc = WideVal<V>::sentinel;  // tsp.cpp:453 (candidates are < INT_MAX by validation)
#pragma unroll
            for (int j = 0; j < T; ++j) acc = WideVal<V>::vmin(acc, g[j] + dl[(m[j] + 1) * n + (k + 1)]);
            const long long rs = hi + lo + B[k][cb + 1];
            tab[os + (unsigned long long)cb * cs + (unsigned long long)rs] = acc;
        }
    }
}

// closing min + backtracking (one wave): lane m-1 holds candidate m
template <typename V>
__global__ void wide_close(const V *__restrict__ dist, int N, const WideInfo *__restrict__ info,
                           const V *__restrict__ tab, V *__restrict__ cost_out, int32_t *__restrict__ tour)
{
    using W = WideVal<V>;
    const int n = N + 1;
    const int lane = threadIdx.x;
    const int m = lane + 1;
    const bool valid = m <= N;
    auto rank_of = [&](uint32_t M) {
        long long r = 0;
        int i = 1;
        while (M) {
            r += info->binom[__builtin_ctz(M)][i++];
            M &= M - 1u;
        }
        return r;
    };
    const V glast = valid ? tab[info->off[N] + (unsigned long long)(m - 1) * info->cnt[N]] : V(0);
    const V cand = valid ? glast + dist[m * n] : W::invalid;
    V best = cand;
    best = tspgpu::wave_min_dpp<V>(best);
    best = W::vmin(best, W::sentinel);
    const unsigned long long hit = __ballot(valid && cand == best && cand < W::sentinel);
    const int bestM = hit ? __ffsll(hit) : 0;
    bool ok = bestM != 0;
    uint32_t S = (uint32_t)((1ull << N) - 1ull);
    int k = bestM;
    int pos = n - 2;
    V target = __shfl(glast, ok ? bestM - 1 : 0);
    while (ok && __builtin_popcount(S) >= 2) {
        const uint32_t T = S & ~(1u << (k - 1));
        const int tt = __builtin_popcount(T);
        const long long rT = rank_of(T);
        const bool inT = valid && ((T >> (m - 1)) & 1u);
        V gv = V(0), c = V(0);
        if (inT) {
            const int j = __builtin_popcount(T & ((1u << (m - 1)) - 1u));
            gv = tab[info->off[tt] + (unsigned long long)j * info->cnt[tt] + (unsigned long long)rT];
            c = gv + dist[m * n + k];
        }
        const unsigned long long bb = __ballot(inT && c == target);
        const int pick = bb ? __ffsll(bb) : 0;
        ok = pick != 0;
        if (lane == 0) tour[pos] = pick;
        target = __shfl(gv, ok ? pick - 1 : 0);
        --pos;
        S = T;
        k = pick;
    }
    if (lane == 0) {
        tour[0] = 0;
        tour[n - 1] = bestM;
        tour[n] = 0;
        *cost_out = ok ? best : W::failed;
    }
}

// Device buffers of one table size and value type, kept in the context
// between calls (tab, dist and cost hold values of type `dtype`).
// (A hipGraph capture of the N launches was measured: same device time,
// the ~8 us per layer at small n is the kernel boundary itself.)
struct WideState {
    int N = 0;
    int dtype = -1;  // TSPGPU_F64 / TSPGPU_I32
    tspgpu::DevBuf<void> tab, dist, cost;
    tspgpu::DevBuf<int32_t> tour;
    tspgpu::DevBuf<WideInfo> info;
    tspgpu::Event e0, e1;
};

// (the context's deleter for wide_cache: either translation unit's copy frees
// a state of either type)
inline void wide_state_free(void *p) { delete static_cast<WideState *>(p); }

template <typename V>
void launch_push(int t, int grid, hipStream_t st, const V *dist, int N, const WideInfo *info, V *tab)
{
    switch (t) {
#define TSPGPU_PUSH(TT) \
    case TT: hipLaunchKernelGGL((wide_push<V, TT>), dim3(grid), dim3(kWideThreads), 0, st, dist, N, info, tab); break;
    TSPGPU_PUSH(1) TSPGPU_PUSH(2) TSPGPU_PUSH(3) TSPGPU_PUSH(4) TSPGPU_PUSH(5) TSPGPU_PUSH(6) TSPGPU_PUSH(7)
    TSPGPU_PUSH(8) TSPGPU_PUSH(9) TSPGPU_PUSH(10) TSPGPU_PUSH(11) TSPGPU_PUSH(12) TSPGPU_PUSH(13) TSPGPU_PUSH(14)
    TSPGPU_PUSH(15) TSPGPU_PUSH(16) TSPGPU_PUSH(17) TSPGPU_PUSH(18) TSPGPU_PUSH(19) TSPGPU_PUSH(20) TSPGPU_PUSH(21)
    TSPGPU_PUSH(22) TSPGPU_PUSH(23) TSPGPU_PUSH(24) TSPGPU_PUSH(25) TSPGPU_PUSH(26) TSPGPU_PUSH(27) TSPGPU_PUSH(28)
    TSPGPU_PUSH(29)
#undef TSPGPU_PUSH
    default: break;
    }
}

// layer 1, layers 2..N, closing + backtracking
template <typename V>
void enqueue_wide(const WideState *w, const WideInfo &h, int n, int cus, hipStream_t st)
{
    const int N = n - 1;
    V *tab = static_cast<V *>(w->tab.p);
    const V *dist = static_cast<const V *>(w->dist.p);
    V *cost = static_cast<V *>(w->cost.p);
    hipLaunchKernelGGL(wide_layer1<V>, dim3(1), dim3(64), 0, st, dist, n, tab);
    // per-destination (pull) form up to 17 cities, where both are bound by the
    // ~8 us kernel boundary per layer and pull is a little faster; the knob
    // WIDE_PULL = 0 / 1 forces either (measured: profiles/r01/k1wide_push_vs_pull.log)
    const bool pull = tspgpu::tuned_or("WIDE_PULL", n <= 17 ? 1 : 0) != 0;
    if (!pull) {
        for (int t = 1; t < N; ++t) {
            const unsigned long long blocks = (h.cnt[t] + kWideThreads - 1) / kWideThreads;
            const unsigned long long cap = (unsigned long long)cus * 16;
            const int grid = (int)(blocks < cap ? blocks : cap);
            launch_push<V>(t, grid, st, dist, N, w->info.p, tab);
        }
        hipLaunchKernelGGL(wide_close<V>, dim3(1), dim3(64), 0, st, dist, N, w->info.p, tab, cost, w->tour.p);
        return;
    }
    for (int s = 2; s <= N; ++s) {
        const unsigned long long total = h.cnt[s] * (unsigned long long)s;
        const unsigned long long blocks = (total + kWideThreads - 1) / kWideThreads;
        const unsigned long long cap = (unsigned long long)cus * 16;
        const int grid = (int)(blocks < cap ? blocks : cap);
        hipLaunchKernelGGL(wide_layer<V>, dim3(grid), dim3(kWideThreads), 0, st, dist, N, w->info.p, s, tab);
    }
    hipLaunchKernelGGL(wide_close<V>, dim3(1), dim3(64), 0, st, dist, N, w->info.p, tab, cost, w->tour.p);
}

// One validated instance (3 <= n <= 31, values checked by the caller) on the
// context's GPU.  The workspace cached in the context is keyed by (N, value
// type): any other key reallocates, sized in bytes of sizeof(V).
template <typename V>
int solve_wide(tspgpu_ctx *c, const V *dist, int n, V *cost_out, int32_t *tour_out, double *kernel_ms)
{
    const int N = n - 1;
    WideInfo h;
    std::memset(&h, 0, sizeof h);
    for (int a = 0; a <= kWideMaxN + 1; ++a) {
        h.binom[a][0] = 1;
        for (int b = 1; b <= a; ++b) h.binom[a][b] = h.binom[a - 1][b - 1] + (b <= a - 1 ? h.binom[a - 1][b] : 0);
    }
    unsigned long long off = 0;
    for (int t = 1; t <= N; ++t) {
        h.cnt[t] = (unsigned long long)h.binom[N][t];
        h.off[t] = off;
        off += h.cnt[t] * (unsigned long long)t;
    }
    const size_t tab_bytes = (size_t)off * sizeof(V);
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    hipStream_t st = c->stream;
    WideState *w = static_cast<WideState *>(c->wide_cache.get());
    std::unique_ptr<WideState> mine;  // a state this call owns: too large to keep
    if (!w || w->N != N || w->dtype != WideVal<V>::dtype) {
        c->wide_cache.reset();
        size_t freeb = 0, totalb = 0;
        if (hipMemGetInfo(&freeb, &totalb) == hipSuccess && tab_bytes + (64u << 20) > freeb) return -ENOMEM;
        mine.reset(w = new (std::nothrow) WideState());
        if (!w) return -ENOMEM;
        w->N = N;
        w->dtype = WideVal<V>::dtype;
        int rc = tspgpu::dev_reserve(w->tab, tab_bytes);
        if (!rc) rc = tspgpu::dev_reserve(w->dist, sizeof(V) * n * n);
        if (!rc) rc = tspgpu::dev_reserve(w->info, sizeof(WideInfo));
        if (!rc) rc = tspgpu::dev_reserve(w->cost, sizeof(V));
        if (!rc) rc = tspgpu::dev_reserve(w->tour, sizeof(int32_t) * (n + 1));
        if (rc) return rc;
        hipError_t e = xcopy_async(w->info, &h, sizeof h, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventCreate(&w->e0.p);
        if (e == hipSuccess) e = hipEventCreate(&w->e1.p);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return tspgpu::hip_err(e);
        // keep small tables for the next call; free >1 GB ones after use
        if (tab_bytes <= ((size_t)1 << 30)) c->wide_cache = tspgpu_erased(mine.release(), wide_state_free);
    }
    hipError_t e = xcopy_async(w->dist, dist, sizeof(V) * n * n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipEventRecord(w->e0, st);
        enqueue_wide<V>(w, h, n, c->cu_count, st);
        c->wide_last_dtype = WideVal<V>::dtype;
        (void)hipEventRecord(w->e1, st);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = xcopy_async(cost_out, w->cost, sizeof(V), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = xcopy_async(tour_out, w->tour, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && kernel_ms) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, w->e0, w->e1) == hipSuccess) *kernel_ms = ms;
    }
    if (e != hipSuccess) return tspgpu::hip_err(e);
    return *cost_out < 0 ? -EIO : 0;
}

}  // namespace tspgpu_wide
