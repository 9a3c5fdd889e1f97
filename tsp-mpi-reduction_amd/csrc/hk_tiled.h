// K1 "sub-cube" Held-Karp: the table layout, the per-block slot format and the
// backtracking kernel that the forward kernel of variant 6 (hk_sub.h) builds on.
//
// Same recurrence, same IEEE operations and the same first-strict-minimum
// argmin as heldkarp_impl.h (tsp.cpp:424-499), so the same cost and tour bits;
// only the order in which DP entries are produced and where they live change.
//
// Split the N inner cities into L "low" ones (bits 0..L-1) and H = N-L "high"
// ones.  A state mask S = h<<L | l has a high part h (H bits) and a low part l.
// The transition G[S\k][m] -> G[S][k] adds ONE city k:
//   * k low:  S\k has the same high part h          -> stays in sub-cube h
//   * k high: S\k has high part h\k (a smaller one) -> crosses sub-cubes
// So the DP can run sub-cube by sub-cube (h = 0, 1, ..., 2^H-1: every h\k is
// done before h), and inside a sub-cube layer by layer over |l| = j.  The
// entries G[S][m] with m LOW never leave the workgroup's LDS (only the two
// live low layers of the current sub-cube are kept: 20 KB at L = 10); only
// the entries with m HIGH go through memory, written once by sub-cube h\m
// ("push", coalesced: same row index l on both sides) and read once by
// sub-cube h.  At n = 16 with the default L = 10 (N = 15, H = 5) that is
// 81,920 of the block's 245,760 entries: 1.31 MB of table traffic per block
// instead of 3.93 MB (SURVEY.md §8(d)'s compulsory bytes of the
// layer-by-layer form).  With L = 11 (H = 4: the 16-city f64 default since
// configuration 65 of k1_cfg.h) it is 65,536 entries, 64 push columns of 2048
// rows, and the two live low layers take 40 KB.
//
// Slot of one block (global memory, tiled_slot_bytes): the push area
// [h][high city][row], the parent words [h][row] and the backtracking's
// recompute area.  The forward kernel keeps the argmin (the reference's first
// strict minimum over members ascending) only for the top rows (>= N -
// TSPGPU_TILED_TA_OFF members: one 64-bit word of 4-bit parents per row);
// everywhere else its pass is min-only — two VALU instructions per relaxation
// instead of four.  The backtracking kernel (hk_tiled_backtrack, one wave per
// block, all blocks at once) follows the parent words down to that size, then
// recomputes the few rows the path still needs from the block's pushed values
// (only subsets of the path's row, 2-8% of the forward relaxations) and takes
// the same first strict minimum of the same candidates — so the same tour
// bits (profiles/r02/k1_argmin_threshold.txt).
//
// The forward kernel this file was written for, variant 5 (a row-owner pass
// per (h, j)), lost to variant 6 at every size and was last in commit
// 8f46298; DESIGN.md §4.0 keeps its measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "heldkarp_impl.h"

namespace tspgpu {

constexpr int kTiledMaxL = 12;
// distance row stride (entries): the per-lane gathers d[m][k] of a half-wave
// fall on bank pair (m * stride + k) mod 32.  16 made every pair m, m+2
// collide (94% bank-conflict cycles); a bank model over every pass's
// (member, destination) positions gives 0.44 extra cycles per low-low gather
// at 17, 0.065 at 19; measured at n = 16 (cfg 14, 4096 blocks,
// profiles/r02/lds_conflicts_stride.txt): conflict cycles 29.7 K -> 20.2 K
// per block (0.575 -> 0.391 of LDS-active cycles), time equal or 0.5% less.
// The rest are the scattered next-layer stores and rank lookups.
#ifndef TSPGPU_TILED_DS
#define TSPGPU_TILED_DS 19
#endif
constexpr int kTiledDS = TSPGPU_TILED_DS;
// Rows with at least N - TSPGPU_TILED_TA_OFF members keep the argmin (a
// 64-bit parent word each); every smaller row is relaxed without it and the
// backtracking recomputes the few rows it needs (see tiled_backtrack).
#ifndef TSPGPU_TILED_TA_OFF
#define TSPGPU_TILED_TA_OFF 4
#endif

// host-built tables of one L (device copy, staged into LDS per workgroup)
struct TiledInfo {
    uint16_t mask[1 << kTiledMaxL];  // L-bit masks sorted by (popcount, colex rank)
    uint16_t rank[1 << kTiledMaxL];  // colex rank of a mask among the masks of its popcount
    uint16_t rankb8[1 << kTiledMaxL];  // rank x 8, rank x 4: byte offsets inside a push / layer column
    uint16_t rankb4[1 << kTiledMaxL];
    int moff[kTiledMaxL + 2];        // first index of popcount class j in mask[]
    int cnt[kTiledMaxL + 2];         // C(L, j)
};

__host__ __device__ constexpr int tiled_layer_vals(int L, int j) { return cbinom(L, j) * j; }
// one LDS region holds the two live low layers: layer j at the bottom when j
// is even, at the top when odd (adjacent layers never overlap)
__host__ __device__ constexpr int tiled_region_vals(int L)
{
    int m = 0;
    for (int j = 0; j < L; ++j) {
        const int s = tiled_layer_vals(L, j) + tiled_layer_vals(L, j + 1);
        m = s > m ? s : m;
    }
    return m;
}
// push area of one slot: [h][c][idx] values (c = high city index 0..H-1,
// idx = the row's place in the sorted L-bit mask list)
__host__ __device__ constexpr size_t tiled_push_bytes(int N, int L, int vb)
{
    return (size_t)(1 << (N - L)) * (N - L) * (1 << L) * vb;
}
// parent words of the workgroup's current block: [h][idx] u64 (only rows
// with >= N - TSPGPU_TILED_TA_OFF members are written)
__host__ __device__ constexpr size_t tiled_parent_bytes(int N, int L)
{
    return TSPGPU_TILED_TA_OFF > 0 ? (size_t)8 << N : 0;
}
// backtracking recompute area: G[h<<L | l][m] of one sub-cube h, [l][m], m low
__host__ __device__ constexpr size_t tiled_recomp_bytes(int L, int vb) { return (size_t)(1 << L) * L * vb; }
// one block's global slot: push area, parent words, recompute area (kept
// until the backtracking kernel has run: one slot per block of a launch)
__host__ __device__ constexpr size_t tiled_slot_bytes(int N, int L, int vb)
{
    return tiled_push_bytes(N, L, vb) + tiled_parent_bytes(N, L) + ((tiled_recomp_bytes(L, vb) + 255) & ~(size_t)255);
}

// f(std::integral_constant<int, 0>), ..., f(std::integral_constant<int, C-1>)
template <int I, int C, typename F>
__device__ __forceinline__ void static_for_impl(F &&f)
{
    if constexpr (I < C) {
        f(std::integral_constant<int, I>{});
        static_for_impl<I + 1, C>(f);
    }
}
template <int C, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    static_for_impl<0, C>(f);
}

__host__ __device__ constexpr int tiled_moff(int L, int J)
{
    int o = 0;
    for (int i = 0; i < J; ++i) o += cbinom(L, i);
    return o;
}

// Buffer-resource access with the uniform part of the offset in soffset (an
// SGPR) and the per-lane part in voffset: no VALU address arithmetic.
// (cache-policy bits of the pushes' loads and stores: A/B builds only)
#ifndef TSPGPU_RS_LOAD_AUX
#define TSPGPU_RS_LOAD_AUX 0
#endif
#ifndef TSPGPU_RS_STORE_AUX
#define TSPGPU_RS_STORE_AUX 0
#endif
template <typename V>
struct Rsrc {
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ V load(uint32_t voff, uint32_t soff) const
    {
        if constexpr (sizeof(V) == 8)
            return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, (int)soff,
                                                                                  TSPGPU_RS_LOAD_AUX));
        else
            return (V)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, TSPGPU_RS_LOAD_AUX);
    }
    __device__ __forceinline__ void store(uint32_t voff, uint32_t soff, V v) const
    {
        if constexpr (sizeof(V) == 8) {
            using u2 = decltype(__builtin_amdgcn_raw_buffer_load_b64(rs, 0, 0, 0));
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), rs, (int)voff, (int)soff,
                                                  TSPGPU_RS_STORE_AUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v, rs, (int)voff, (int)soff, TSPGPU_RS_STORE_AUX);
        }
    }
    // non-temporal 8-byte store (parent words: read back only by the backtracking)
    __device__ __forceinline__ void store_nt(uint32_t voff, uint32_t soff, uint64_t w) const
    {
        using u2 = decltype(__builtin_amdgcn_raw_buffer_load_b64(rs, 0, 0, 0));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, w), rs, (int)voff, (int)soff, 2);
    }
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void *p, uint32_t bytes)
{
    const uint64_t base = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    const uint32_t nb = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), 0, (int)nb,
                                             0x00020000);
}

// LDS barrier: the passes inside a sub-cube hand data over through LDS only
// (their pushes are read by later sub-cubes, behind a full __syncthreads), so
// they wait for their own LDS operations, not for their global stores.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// acc = min(acc, g + d) with arg = m where g + d < acc (the first strict
// minimum over members ascending, tsp.cpp:465): exactly four VALU
// instructions with the compare in VCC (compiler-scheduled compares landed in
// SGPR pairs that were spilled, round-1 K1 counters).
__device__ __forceinline__ void relax_argmin(double &acc, uint32_t &arg, double g, double d, uint32_t m)
{
    double t;
    asm volatile(
        "v_add_f64 %[t], %[g], %[d]\n\t"
        "v_cmp_lt_f64 vcc, %[t], %[acc]\n\t"
        "v_cndmask_b32 %[arg], %[arg], %[m], vcc\n\t"
        "v_min_f64 %[acc], %[acc], %[t]"
        : [acc] "+v"(acc), [arg] "+v"(arg), [t] "=&v"(t)
        : [g] "v"(g), [d] "v"(d), [m] "v"(m)
        : "vcc");
}
__device__ __forceinline__ void relax_argmin(int32_t &acc, uint32_t &arg, int32_t g, int32_t d, uint32_t m)
{
    int32_t t;
    asm volatile(
        "v_add_u32 %[t], %[g], %[d]\n\t"
        "v_cmp_lt_i32 vcc, %[t], %[acc]\n\t"
        "v_cndmask_b32 %[arg], %[arg], %[m], vcc\n\t"
        "v_min_i32 %[acc], %[acc], %[t]"
        : [acc] "+v"(acc), [arg] "+v"(arg), [t] "=&v"(t)
        : [g] "v"(g), [d] "v"(d), [m] "v"(m)
        : "vcc");
}

// acc = min(acc, g + d), no argmin (ablation 8 / argmin-free passes)
__device__ __forceinline__ void relax_min(double &acc, double g, double d)
{
    double t;
    asm volatile("v_add_f64 %[t], %[g], %[d]\n\tv_min_f64 %[acc], %[acc], %[t]"
                 : [acc] "+v"(acc), [t] "=&v"(t)
                 : [g] "v"(g), [d] "v"(d));
}
__device__ __forceinline__ void relax_min(int32_t &acc, int32_t g, int32_t d)
{
    int32_t t;
    asm volatile("v_add_u32 %[t], %[g], %[d]\n\tv_min_i32 %[acc], %[acc], %[t]"
                 : [acc] "+v"(acc), [t] "=&v"(t)
                 : [g] "v"(g), [d] "v"(d));
}

template <typename V, int N, int L, int R>
struct TiledCtx {
    const V *dr;               // LDS distances, rows of kTiledDS entries, R copies each (R = 1 in use)
    const uint16_t *lmask;     // sorted L-bit masks (LDS)
    const uint16_t *lrankb;    // colex rank x sizeof(V) (byte offset inside a position column)
    V *region;                 // LDS live low layers
    Rsrc<V> push;              // this slot's push area
    Rsrc<uint64_t> par;        // this slot's parent words (the current block's)
    Rsrc<V> rec;               // this slot's backtracking recompute area
    const int *moff;           // first index of each popcount class (backtracking)
};

__host__ __device__ constexpr int pow2_at_least(int q)
{
    int p = 1;
    while (p < q) p *= 2;
    return p;
}

// Parallel bit deposit: the i-th set bit of m receives bit i of x.
__device__ __forceinline__ uint32_t pdep_u32(uint32_t x, uint32_t m)
{
    uint32_t r = 0;
    for (uint32_t b = 1; m; b <<= 1) {
        const uint32_t low = m & (0u - m);
        if (x & b) r |= low;
        m ^= low;
    }
    return r;
}

// G[h<<L | l][m] after the forward pass: a high m from the push area, a low m
// from the recompute area (valid for the sub-cube and the subsets the last
// tiled_recompute covered).  Any m < N gives a valid address (the value of a
// non-member is garbage): callers load unconditionally, then select.
template <typename V, int N, int L, int R>
__device__ __forceinline__ V tiled_g(const TiledCtx<V, N, L, R> &c, uint32_t h, uint32_t l, uint32_t pidx, int m)
{
    constexpr int H = N - L, NL = 1 << L, VB = sizeof(V);
    if (m < L) return c.rec.load((l * L + (uint32_t)m) * VB, 0);
    return c.push.load(pidx, (h * H + (uint32_t)(m - L)) * (uint32_t)(NL * VB));
}
// byte offset of row l inside a push column
template <typename V, int N, int L, int R>
__device__ __forceinline__ uint32_t tiled_pidx(const TiledCtx<V, N, L, R> &c, uint32_t l)
{
    return (uint32_t)c.moff[__builtin_popcount(l)] * (uint32_t)sizeof(V) + c.lrankb[l];
}

// Backtracking recompute (one wave): G[h<<L | l'][m] for every l' within lT and
// every low member m, layer by layer from the pushed high-member values — the
// forward pass's own relaxations restricted to those rows, the minimum only
// (IEEE min is order-free, so the values are the forward pass's bits).
// Round 6: a lane per (row, destination) pair — a layer of C(nl, j) rows has
// (nl - j) destinations per row, so a wave's lanes are busy where the
// row-per-lane form left most idle in the small layers, and each lane relaxes
// only its own destination over the row's members only (not N predicated
// relaxations per possible destination): hk_tiled_backtrack per 65536 16-city
// blocks 1.76 ms (row per lane) -> 1.44 ms (pairs) -> ~1.33 ms (members
// only; profiles/r06/bt_ab.txt).
template <typename V, int N, int L, int R>
__device__ void tiled_recompute(const TiledCtx<V, N, L, R> &c, const V *d0, uint32_t h, uint32_t lT,
                                uint32_t lane)
{
    constexpr int VB = sizeof(V);
    const int nl = __builtin_popcount(lT);
    const int hcnt = __builtin_popcount(h);
    int j0 = 0;
    if (h == 0) {  // no high member: layer 1 is G[{k}][k] = d[0][k] (tsp.cpp:435)
        if (lane < (uint32_t)L && ((lT >> lane) & 1u)) c.rec.store(((1u << lane) * L + lane) * VB, 0, d0[lane]);
        j0 = 1;
    }
    for (int j = j0; j < nl; ++j) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int q = nl - j, pairs = cbinom(nl, j) * q, mo = c.moff[j];
        for (int e = (int)lane; e < pairs; e += 64) {
            const int r = e / q, qi = e - r * q;
            // the r-th j-subset of lT in colex order = the r-th j-subset of
            // the low bits, deposited on lT's cities; its qi-th destination
            const uint32_t lp = pdep_u32(c.lmask[mo + r], lT);
            const uint32_t s = (uint32_t)__builtin_ctz(pdep_u32(1u << qi, lT & ~lp));
            const uint32_t Tm = (h << L) | lp;
            const uint32_t pidx = tiled_pidx(c, lp);
            // members only: the row's T = j + |h| members (T wave-uniform, so
            // every "q < T" is a scalar branch), their loads all in flight
            // (round 6: -7.5% against N predicated relaxations per pair)
            const int T = j + hcnt;
            V acc = ValT<V>::inf;
            // (every value in flight at once: 9 VGPRs of spills at six
            // workgroups per CU, and still faster than loading the member
            // list in two halves without spills, 0.41 vs 0.51 ms per 16384
            // blocks: profiles/r06/bt_ab.txt)
            V gv[N - 1];
            uint32_t x = Tm;
#pragma unroll
            for (int q = 0; q < N - 1; ++q) {
                if (q < T) gv[q] = tiled_g(c, h, lp, pidx, __builtin_ctz(x));
                x &= x - 1u;
            }
            x = Tm;
#pragma unroll
            for (int q = 0; q < N - 1; ++q) {
                if (q < T) acc = ValT<V>::vmin(acc, gv[q] + c.dr[((uint32_t)__builtin_ctz(x) * kTiledDS + s) * R]);
                x &= x - 1u;
            }
            c.rec.store(((lp | (1u << s)) * L + s) * VB, 0, acc);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Backtracking of the block just solved (one wave, tsp.cpp:473-481's parent
// walk): from the last inner city k_last back to the start.  A row with
// >= N - TSPGPU_TILED_TA_OFF members has its parent word; below that the row's
// values are recomputed (tiled_recompute, once per sub-cube the path enters)
// and the parent is the first strict minimum over its members ascending of
// G[T][m] + d[m][k] — the forward pass's candidates, so its argmin.
template <typename V, int N, int L, int R>
__device__ bool tiled_backtrack(const TiledCtx<V, N, L, R> &c, const V *d0, int bestM,
                                int32_t *tour, uint32_t lane)
{
    constexpr int NL = 1 << L, VB = sizeof(V), n = N + 1;
    uint32_t S = (1u << N) - 1u;
    int k = bestM - 1;
    bool ok = bestM >= 1 && bestM <= N;
    uint32_t hcur = ~0u, lcur = 0;
    for (int pos = n - 2; ok && pos >= 1; --pos) {
        const uint32_t T = S & ~(1u << k);
        const uint32_t hT = T >> L, lT = T & (uint32_t)(NL - 1);
        int pm;
        if (__builtin_popcount(T) >= N - TSPGPU_TILED_TA_OFF) {
            const uint32_t idx = (uint32_t)c.moff[__builtin_popcount(lT)] + c.lrankb[lT] / VB;
            const uint64_t w = c.par.load(idx * 8u, hT * (uint32_t)(NL * 8));
            const int q = k - __builtin_popcount(T & ((1u << k) - 1u));  // k's place among T's non-members
            pm = (int)((w >> (4 * q)) & 15u);
        } else {
            if (hT != hcur || (lT & ~lcur)) {
                tiled_recompute(c, d0, hT, lT, lane);
                hcur = hT;
                lcur = lT;
            }
            const bool mem = lane < (uint32_t)N && ((T >> lane) & 1u);
            V cand = ValT<V>::invalid;
            const V g = tiled_g(c, hT, lT, tiled_pidx(c, lT), lane < (uint32_t)N ? (int)lane : 0);
            if (mem) cand = g + c.dr[(lane * kTiledDS + (uint32_t)k) * R];
            const V best = wave_min(cand);
            const unsigned long long hit = __ballot(mem && cand == best);
            pm = hit ? __ffsll(hit) - 1 : N;
        }
        ok = pm < N && ((T >> pm) & 1u);
        if (lane == 0) tour[pos] = ok ? pm + 1 : 0;
        S = T;
        k = pm;
    }
    return ok;
}

// waves per SIMD of a forward kernel with wg_per_cu workgroups of `threads` on a CU (__launch_bounds__)
__host__ __device__ constexpr int tiled_waves(int threads, int wg_per_cu) { return threads * wg_per_cu / 256; }

// Backtracking (tiled_backtrack): one wave per block, four per workgroup,
// persistent over the blocks of the launch.  A block's backtracking is a chain
// of dependent loads (tens of microseconds), so all resident waves run their
// chains at the same time, after the forward kernel instead of stalling it.
constexpr int kTiledBtWaves = 4;
#ifndef TSPGPU_TILED_BTWG
#define TSPGPU_TILED_BTWG 6  // backtracking workgroups per CU (register budget)
#endif
namespace {  // internal linkage: every instantiation file keeps its own (timing builds differ per file)
template <typename V, int N, int L>
__global__ __launch_bounds__(64 * kTiledBtWaves, TSPGPU_TILED_BTWG) void hk_tiled_backtrack(
    int nblocks, int blk0, const char *__restrict__ slots, uint32_t slot_bytes, const TiledInfo *__restrict__ info,
    const V *__restrict__ dist, V *__restrict__ cost_out, int32_t *__restrict__ tour_out)
{
    constexpr int NL = 1 << L, n = N + 1, VB = sizeof(V), DRV = N * kTiledDS + 16;
    __shared__ uint16_t lmask[NL], lrankb[NL];
    __shared__ int smoff[L + 2];
    __shared__ V drs[kTiledBtWaves][DRV];     // per wave: the block's inner distances, then d[0][k]
    for (int i = threadIdx.x; i < NL; i += 64 * kTiledBtWaves) {
        lmask[i] = info->mask[i];
        lrankb[i] = (uint16_t)(info->rank[i] * VB);
    }
    if (threadIdx.x < (uint32_t)(L + 2)) smoff[threadIdx.x] = info->moff[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    V *dr = drs[wave];
    TiledCtx<V, N, L, 1> c;
    c.dr = dr;
    c.lmask = lmask;
    c.lrankb = lrankb;
    c.region = nullptr;
    c.moff = smoff;
    for (int blk = blk0 + (int)(blockIdx.x * kTiledBtWaves + wave); blk < nblocks;
         blk += (int)(gridDim.x * kTiledBtWaves)) {
        const V *dsrc = dist + (size_t)blk * n * n;
        for (int i = lane; i < N * kTiledDS; i += 64) {
            const int m = i / kTiledDS, k = i % kTiledDS;
            dr[i] = k < N ? dsrc[(m + 1) * n + (k + 1)] : V(0);
        }
        if (lane < (uint32_t)N) dr[N * kTiledDS + lane] = dsrc[lane + 1];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        int32_t *tour = tour_out + (size_t)blk * (n + 1);
        const int bestM = tour[n - 1];
        if (bestM < 1) continue;  // no tour (cost already -1)
        char *slot = const_cast<char *>(slots) + (size_t)(blk - blk0) * slot_bytes;
        c.push.rs = uniform_rsrc(slot, (uint32_t)tiled_push_bytes(N, L, VB));
        c.par.rs = uniform_rsrc(slot + tiled_push_bytes(N, L, VB), (uint32_t)tiled_parent_bytes(N, L));
        c.rec.rs = uniform_rsrc(slot + tiled_push_bytes(N, L, VB) + tiled_parent_bytes(N, L),
                                (uint32_t)tiled_recomp_bytes(L, VB));
        if (!tiled_backtrack(c, dr + N * kTiledDS, bestM, tour, lane) && lane == 0) cost_out[blk] = V(-1);
        __builtin_amdgcn_wave_barrier();  // dr is reloaded for the next block
    }
}
}  // namespace

}  // namespace tspgpu
