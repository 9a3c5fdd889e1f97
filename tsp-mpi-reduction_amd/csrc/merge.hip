// K3 — the reference's mergeBlocks (tsp.cpp:197-269) and its reduction tree
// (tsp.cpp:52-134, 348-352) with the paths resident on the GPU.
//
// mergeBlocks looks for the pair of edges (A,B) of path 1 and (C,D) of path 2
// (cyclic successors, the closing duplicate city included) with the smallest
//     swapPairCost = ((d(A,D) + d(B,C)) - d(A,B)) - d(C,D)        (tsp.cpp:197-200)
// first strict minimum in row-major (i, j) order from INT_MAX (tsp.cpp:204-227),
// then splices path 2 (closing city dropped, rotated to start after C,
// reversed) behind the first city of path 1 that is A or B (tsp.cpp:229-259).
// The reference is O(L1 * L2^2) (it rotates a vector per step); the search is
// an L1 x L2 argmin, i.e. GPU work once the running path grows (a rank folds
// all its blocks into one path, so at ./tsp 16 16384 the fold alone is ~4e10
// pair evaluations).
//
// Exactness.  d() is sqrt(pow(dx,2) + pow(dy,2)) with glibc pow, which differs
// from dx*dx in ~0.08% of inputs, so the device cannot reproduce d() bit for
// bit.  It computes every swap cost with dx*dx (a few ulp from the glibc
// value) and keeps as candidates all pairs within 2*eps of its minimum, eps =
// 2^-36 * 4 * Dmax (Dmax: the diagonal of the cities' bounding box) — about
// 10^4 times the largest possible discrepancy.  The host re-evaluates the
// candidates with glibc pow, in row-major order, with the reference's strict
// <: the exact minimum and every pair tied with it are always among them.
// If there are more candidates than the buffer holds, the host scans all
// pairs itself.  The splice is a gather kernel; the first-occurrence searches
// it needs are atomicMin reductions.  One host round trip per merge.
//
// The reduction has one core and two fronts.  reduce_core
// works on block paths in device memory and can leave rank 0's final path
// (the merged tour) in host or device memory.  reduce_host (tspgpu_reduce,
// tspgpu_reduce_path) scans host paths and uploads them; tspgpu_reduce_device
// takes K1's outputs where tspgpu_solve_cities_device left them: paths.hip
// gathers the paths and brings the same facts, so only the costs visit the
// host.  tspgpu_pipeline_cities chains upload, K1 and that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "abi_internal.h"
#include "ctx.h"
#include "paths.h"
#include "xfer.h"
#include "tuning.h"
#include "wave.h"
#include "tspgpu.h"

using tspgpu::DevBuf;
using tspgpu::hip_err;
using tspgpu::Pinned;
using tspgpu::xcopy_async;

namespace {

constexpr int kMergeThreads = 256;
constexpr unsigned kCandCap = 1u << 16;
constexpr int kChunk = 1024;       // path-2 cities staged in LDS per block column
constexpr int kBatch = 2048;       // merges in flight between two host synchronisations
constexpr int kMaxBlocks = 4096;   // argmin / candidate grid (per-block minima kept)

struct Cand {
    int i, j;
    tspgpu_city a, b, c, d;
};

// Device control words of the merge stream.
struct Ctl {
    unsigned long long count;     // candidates of the current merge
    unsigned long long minkey;    // min order key of its swap costs
    unsigned long long done;      // candidate blocks finished (last block decides)
    unsigned long long stall;     // 0 ok; 1 the host must pick (several candidates); 2 EDEADLK; 3 EIO
    unsigned long long stall_at;  // batch index of the merge that stalled
    unsigned long long fw[2];     // first index of A|B in path 1, of C in path 2
    unsigned long long pad;
};

// What each merge leaves for the host: the chosen pair (the exact swap cost
// is recomputed with glibc pow on the host, tsp.cpp:263).
struct Pick {
    Cand c;
};

__device__ __forceinline__ double ddist(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx;
    const double dy = ay - by;
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ unsigned long long order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__host__ __device__ __forceinline__ double key_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __builtin_bit_cast(double, b);
}

// Stage path-2 cities [j0, j0 + J] (successor included, cyclic) and the path-2
// edge lengths d(C_j, D_j) in LDS.
struct Stage {
    double x[kChunk + 1], y[kChunk + 1], e[kChunk];
};
__device__ __forceinline__ int stage_chunk(Stage &sm, const tspgpu_city *c2, int L2, int j0, int cw = kChunk)
{
    const int J = min(cw, L2 - j0);
    for (int t = threadIdx.x; t <= J; t += kMergeThreads) {
        const int j = j0 + t;
        const tspgpu_city c = c2[j < L2 ? j : j - L2];
        sm.x[t] = c.x;
        sm.y[t] = c.y;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < J; t += kMergeThreads) sm.e[t] = ddist(sm.x[t], sm.y[t], sm.x[t + 1], sm.y[t + 1]);
    __syncthreads();
    return J;
}

// Approximate swap costs (dx*dx, IEEE sqrt; tsp.cpp:197-200 order of operations)
// of path-1 edge i against the staged path-2 edges; calls f(j, cost).
template <typename F>
__device__ __forceinline__ void sweep_row(const Stage &sm, int J, const tspgpu_city *c1, int L1, int i, F &&f)
{
    const tspgpu_city A = c1[i], B = c1[i + 1 == L1 ? 0 : i + 1];
    const double eab = ddist(A.x, A.y, B.x, B.y);
    for (int t = 0; t < J; ++t) {
        const double sc = ((ddist(A.x, A.y, sm.x[t + 1], sm.y[t + 1]) + ddist(B.x, B.y, sm.x[t], sm.y[t])) - eab) -
                          sm.e[t];
        f(t, sc);
    }
}

// Pass 1: min swap key over all L1 x L2 pairs; blockIdx.y = path-2 chunk.
// Also resets this merge's first-occurrence words for find_kernel.
__global__ __launch_bounds__(kMergeThreads) void argmin_kernel(const tspgpu_city *c1, int L1, const tspgpu_city *c2,
                                                               int L2, int cw, Ctl *ctl, unsigned long long *blockmin)
{
    if (ctl->stall) return;
    __shared__ Stage sm;
    __shared__ unsigned long long wmin[kMergeThreads / 64];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        ctl->fw[0] = ~0ull;
        ctl->fw[1] = ~0ull;
    }
    unsigned long long best = ~0ull;
    for (int j0 = blockIdx.y * cw; j0 < L2; j0 += gridDim.y * cw) {
        const int J = stage_chunk(sm, c2, L2, j0, cw);
        for (int i = blockIdx.x * kMergeThreads + threadIdx.x; i < L1; i += gridDim.x * kMergeThreads)
            sweep_row(sm, J, c1, L1, i, [&](int, double sc) {
                const unsigned long long k = order_key(sc);
                best = k < best ? k : best;
            });
        __syncthreads();  // before the next chunk overwrites the stage
    }
    best = tspgpu::wave_min_dpp(best);
    if (__lane_id() == 0) wmin[threadIdx.x / 64] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = wmin[0];
        for (int w = 1; w < kMergeThreads / 64; ++w) b = wmin[w] < b ? wmin[w] : b;
        blockmin[blockIdx.y * gridDim.x + blockIdx.x] = b;
        if (b != ~0ull) atomicMin(&ctl->minkey, b);
    }
}

// Fold merges (path 2 is one block tour, L2 <= kChunk; path 1 holds each
// city once plus the closing copy of its first city): ONE kernel does both
// passes and the decision.  Every block computes its minimum; the last block
// to finish rescans the blocks within eps2 of the global minimum, and with
// exactly one candidate it logs the pick and the splice positions directly:
// the first city of path 1 that is A or B is index i (0 when A or B is the
// start city), C's first index in path 2 is j (0 for the closing copy).
// Otherwise the stream stalls for the host.
__global__ __launch_bounds__(kMergeThreads) void fold_pick_kernel(const tspgpu_city *c1, int L1, const tspgpu_city *c2,
                                                                  int L2, double eps2, Ctl *ctl,
                                                                  unsigned long long *blockmin, Cand *cand,
                                                                  Pick *picks, int idx)
{
    if (ctl->stall) return;
    __shared__ Stage sm;
    __shared__ unsigned long long wmin[kMergeThreads / 64];
    __shared__ bool last;
    __shared__ unsigned nc;
    const int J = stage_chunk(sm, c2, L2, 0);
    unsigned long long best = ~0ull;
    for (int i = blockIdx.x * kMergeThreads + threadIdx.x; i < L1; i += gridDim.x * kMergeThreads)
        sweep_row(sm, J, c1, L1, i, [&](int, double sc) {
            const unsigned long long k = order_key(sc);
            best = k < best ? k : best;
        });
    best = tspgpu::wave_min_dpp(best);
    if (__lane_id() == 0) wmin[threadIdx.x / 64] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = wmin[0];
        for (int w = 1; w < kMergeThreads / 64; ++w) b = wmin[w] < b ? wmin[w] : b;
        blockmin[blockIdx.x] = b;
        if (b != ~0ull) atomicMin(&ctl->minkey, b);
        __threadfence();
        last = atomicAdd(&ctl->done, 1ull) == (unsigned long long)gridDim.x - 1;
        nc = 0;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    const double thr = key_value(__hip_atomic_load(&ctl->minkey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) + eps2;
    // the blocks within eps2 of the minimum (usually one), gathered in parallel
    __shared__ int close[64];
    __shared__ unsigned nclose;
    if (threadIdx.x == 0) nclose = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kMergeThreads) {
        const unsigned long long bm = __hip_atomic_load(&blockmin[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key_value(bm) <= thr) {
            const unsigned q = atomicAdd(&nclose, 1u);
            if (q < 64) close[q] = b;
        }
    }
    __syncthreads();
    const bool all = nclose > 64;  // (many near-ties: rescan every block)
    const int nb = all ? (int)gridDim.x : (int)nclose;
    for (int q = 0; q < nb; ++q) {
        const int b = all ? q : close[q];
        for (int i = b * kMergeThreads + threadIdx.x; i < L1; i += gridDim.x * kMergeThreads)
            sweep_row(sm, J, c1, L1, i, [&](int t, double sc) {
                if (sc <= thr) {
                    const unsigned s2 = atomicAdd(&nc, 1u);
                    if (s2 < kCandCap) {
                        Cand c;
                        c.i = i;
                        c.j = t;
                        c.a = c1[i];
                        c.b = c1[i + 1 == L1 ? 0 : i + 1];
                        c.c = c2[t];
                        c.d = c2[t + 1 == L2 ? 0 : t + 1];
                        cand[s2] = c;
                    }
                }
            });
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    __threadfence();
    ctl->count = nc;
    if (nc != 1) {
        ctl->stall_at = (unsigned long long)idx;
        ctl->stall = 1;
        return;
    }
    const Cand k = cand[0];
    picks[idx].c = k;
    const int first = c1[0].id;
    ctl->fw[0] = (k.a.id == first || k.b.id == first) ? 0ull : (unsigned long long)k.i;
    ctl->fw[1] = k.j == L2 - 1 ? 0ull : (unsigned long long)k.j;
}

// Pass 2: every pair within eps2 of the minimum is a candidate (only blocks
// whose own minimum is that close rescan; the others return at once).
__global__ __launch_bounds__(kMergeThreads) void cand_kernel(const tspgpu_city *c1, int L1, const tspgpu_city *c2,
                                                             int L2, int cw, double eps2, Ctl *ctl,
                                                             const unsigned long long *blockmin, Cand *cand)
{
    if (ctl->stall) return;
    __shared__ Stage sm;
    const double thr = key_value(ctl->minkey) + eps2;
    if (!(key_value(blockmin[blockIdx.y * gridDim.x + blockIdx.x]) <= thr)) return;
    for (int j0 = blockIdx.y * cw; j0 < L2; j0 += gridDim.y * cw) {
        const int J = stage_chunk(sm, c2, L2, j0, cw);
        for (int i = blockIdx.x * kMergeThreads + threadIdx.x; i < L1; i += gridDim.x * kMergeThreads)
            sweep_row(sm, J, c1, L1, i, [&](int t, double sc) {
                if (sc <= thr) {
                    const unsigned s2 = (unsigned)atomicAdd(&ctl->count, 1ull);
                    if (s2 < kCandCap) {
                        const int j = j0 + t;
                        Cand c;
                        c.i = i;
                        c.j = j;
                        c.a = c1[i];
                        c.b = c1[i + 1 == L1 ? 0 : i + 1];
                        c.c = c2[j];
                        c.d = c2[j + 1 == L2 ? 0 : j + 1];
                        cand[s2] = c;
                    }
                }
            });
        __syncthreads();
    }
}

// first index of path 1 whose id is A or B -> fw[0], first index of path 2
// [0, M) whose id is C -> fw[1] (tsp.cpp:229-239); ids from the pick unless given
// Unforced: exactly one candidate -> it is the reference's pair (the exact
// minimum and all its ties are always inside the window): log it as the
// merge's pick; else stall the stream for the host's exact re-evaluation.
__global__ __launch_bounds__(kMergeThreads) void find_kernel(const tspgpu_city *c1, int L1, const tspgpu_city *c2,
                                                             int M, Ctl *ctl, const Cand *cand, Pick *picks, int idx,
                                                             int idA, int idB, int idC, int forced)
{
    if (ctl->stall && !forced) return;
    if (!forced) {
        __shared__ int ids[4];
        if (threadIdx.x == 0) {
            const bool one = ctl->count == 1;
            ids[3] = one;
            if (one) {
                const Cand k = cand[0];
                ids[0] = k.a.id;
                ids[1] = k.b.id;
                ids[2] = k.c.id;
                if (blockIdx.x == 0) picks[idx].c = k;
            } else if (blockIdx.x == 0) {
                ctl->stall_at = (unsigned long long)idx;
                ctl->stall = 1;
            }
        }
        __syncthreads();
        if (!ids[3]) return;
        idA = ids[0];
        idB = ids[1];
        idC = ids[2];
    }
    const int t = blockIdx.x * kMergeThreads + threadIdx.x;
    const int stride = gridDim.x * kMergeThreads;
    for (int i = t; i < L1; i += stride)
        if (c1[i].id == idA || c1[i].id == idB) atomicMin(&ctl->fw[0], (unsigned long long)i);
    for (int j = t; j < M; j += stride)
        if (c2[j].id == idC) atomicMin(&ctl->fw[1], (unsigned long long)j);
}

// out = c1[0..p] ++ reverse(c2 rotated to start after C, closing city dropped) ++ c1[p+1..]
// (tsp.cpp:240-259), copied as 8-byte words (3 per city); then clears the
// words of the next merge.
__global__ __launch_bounds__(kMergeThreads) void splice_kernel(const tspgpu_city *c1, int L1, const tspgpu_city *c2,
                                                               int M, Ctl *ctl, tspgpu_city *out, int idx, int forced)
{
    static_assert(sizeof(tspgpu_city) == 24, "City layout");
    if (ctl->stall && !forced) return;
    const unsigned long long pw = ctl->fw[0], sw = ctl->fw[1];
    if (pw >= (unsigned long long)L1 || sw >= (unsigned long long)M) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ctl->stall_at = (unsigned long long)idx;
            ctl->stall = sw >= (unsigned long long)M ? 2 : 3;  // C not in path 2: tsp.cpp:236-239 never ends
        }
        return;
    }
    const int p = (int)pw, start = (int)((sw + 1) % (unsigned)M);
    const unsigned long long *w1 = reinterpret_cast<const unsigned long long *>(c1);
    const unsigned long long *w2 = reinterpret_cast<const unsigned long long *>(c2);
    unsigned long long *wo = reinterpret_cast<unsigned long long *>(out);
    const int total = 3 * (L1 + M);
    for (int w = blockIdx.x * kMergeThreads + threadIdx.x; w < total; w += gridDim.x * kMergeThreads) {
        const int k = w / 3, f = w - 3 * k;
        int src;
        const unsigned long long *base;
        if (k <= p) {
            base = w1;
            src = k;
        } else if (k <= p + M) {
            const int q = start + (M - 1 - (k - p - 1));
            base = w2;
            src = q >= M ? q - M : q;
        } else {
            base = w1;
            src = k - M;
        }
        wo[w] = base[3 * src + f];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->count = 0;
        ctl->minkey = ~0ull;
        ctl->done = 0;
        if (forced) ctl->stall = 0;
    }
}

// ---- persistent per-rank fold (tsp.cpp:348-352) --------------------------------
//
// The local fold s = ((b0 ⊕ b1) ⊕ b2) ... of every logical rank's contiguous
// blocks is a chain of small dependent merges (path 1 grows by one block tour
// of M = L2 - 1 cities per merge).  As separate launches it was 2 kernels per
// merge in strict sequence (./tsp 8 1024 at P = 8: 1,016 fold_pick + 1,023
// splice launches, ~10 us each, profiles/r04/k3_kernel_stats.csv).  Here ONE
// launch runs every rank's whole fold: a workgroup per rank keeps its path in
// LDS (structure of arrays), and each merge is three phases between workgroup
// barriers — the swap-cost minimum (dx*dx, IEEE sqrt, the reference's order of
// operations), the candidates within eps2 of it, and, with exactly one
// candidate (then it is the reference's pair, as for fold_pick_kernel), the
// splice in LDS.  The pick (A, B, C, D) of every merge is logged for the
// host's exact cost fold (glibc pow, tsp.cpp:263).  A merge with several
// candidates, or one whose result would not fit the LDS path, stops the rank:
// its path goes to global memory with the index of the merge, for the host
// (exact pick, then the remaining merges by the general path or a relaunch).
constexpr int kFoldThreads = 1024;
constexpr int kFoldCap = 4096;   // cities of a rank's path held in LDS (20 B each)
constexpr int kFoldL2 = 33;      // block tours up to 32 cities + the closing copy

struct FoldJob {
    int first;     // block of the rank's running path when the kernel starts (path = that block's tour if k0 == 0)
    int count;     // blocks of the rank: merges k0 .. count-2 fold blocks first + 1 + k
    int k0;        // next merge (0: start from the block; > 0: from path/len, a relaunch)
    int len;       // running path length when k0 > 0 (in `path`)
    tspgpu_city *path;  // the rank's running path (global; capacity >= all cities)
    Pick *picks;        // one per merge of this rank (count - 1)
};
struct FoldOut {
    int status;  // 0 done, 1 stalled (several candidates) at merge `at`, 2 path cap reached before merge `at`
    int at;
    int len;     // running path length written to path (status != 0: before merge `at`)
    int count;   // candidates of the stalled merge
};

// (key, pair) of the smallest swap cost and the second-smallest key of a set
// of pairs: exactly one pair is within eps2 of the minimum iff the second key
// lies above min + eps2 — one pass over the pairs decides what fold_pick's
// two passes did
struct Top2 {
    unsigned long long k1, k2;
    unsigned i1;
};
__device__ __forceinline__ void top2_add(Top2 &a, unsigned long long k, unsigned i)
{
    if (k < a.k1) {
        a.k2 = a.k1;
        a.k1 = k;
        a.i1 = i;
    } else if (k < a.k2) {
        a.k2 = k;
    }
}
__device__ __forceinline__ Top2 top2_merge(const Top2 &a, const Top2 &b)
{
    Top2 r;
    const bool lo = a.k1 < b.k1 || (a.k1 == b.k1 && a.i1 < b.i1);
    r.k1 = lo ? a.k1 : b.k1;
    r.i1 = lo ? a.i1 : b.i1;
    const unsigned long long hi = lo ? b.k1 : a.k1;
    r.k2 = min(hi, min(a.k2, b.k2));
    return r;
}
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int m)
{
    const int lo = __shfl_xor((int)(unsigned)v, m), hi = __shfl_xor((int)(unsigned)(v >> 32), m);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

//
// kRagged: the blocks differ in length.  Block b then lies at
// blocks + desc[b].path and has desc[b].L cities (block_desc.h) where the
// uniform form has b * L2u and L2u; everything below a merge's first two lines
// works from that merge's own (c2, L2, M) in both forms.
template <bool kRagged>
__global__ __launch_bounds__(kFoldThreads) void fold_persist_kernel(const tspgpu_city *blocks, int L2u,
                                                                    const tspgpu::BlockDesc *desc, double eps2,
                                                                    const FoldJob *jobs, FoldOut *outs)
{
    __shared__ double px[kFoldCap], py[kFoldCap];
    __shared__ int pid[kFoldCap];
    __shared__ double cx[kFoldL2], cy[kFoldL2], ce[kFoldL2];
    __shared__ int cid[kFoldL2];
    __shared__ Top2 wtop[kFoldThreads / 64];
    const FoldJob J = jobs[blockIdx.x];
    const int t = threadIdx.x;
    // block b's cities and length (the same for every thread of the workgroup)
    auto block_at = [&](int b) -> const tspgpu_city * {
        if constexpr (kRagged) return blocks + desc[b].path;
        return blocks + (size_t)b * L2u;
    };
    auto block_len = [&](int b) -> int {
        if constexpr (kRagged) return desc[b].L;
        return L2u;
    };
    int len;
    if (J.k0 == 0) {
        const int L2 = block_len(J.first);
        len = L2;
        const tspgpu_city *b = block_at(J.first);
        for (int k = t; k < L2; k += kFoldThreads) {
            const tspgpu_city c = b[k];
            px[k] = c.x, py[k] = c.y, pid[k] = c.id;
        }
    } else {
        len = J.len;
        for (int k = t; k < len; k += kFoldThreads) {
            const tspgpu_city c = J.path[k];
            px[k] = c.x, py[k] = c.y, pid[k] = c.id;
        }
    }
    int status = 0, at = J.count - 1, nc = 1;
    for (int m = J.k0; m < J.count - 1; ++m) {
        const int L2 = block_len(J.first + 1 + m), M = L2 - 1;
        if (len + M > kFoldCap || L2 > kFoldL2) {  // (the host sends no block above kFoldL2 here)
            status = 2, at = m;
            break;
        }
        // stage the block (cities and edge lengths, read straight from memory:
        // one barrier, which also orders the previous splice's LDS writes)
        const tspgpu_city *c2 = block_at(J.first + 1 + m);
        if (t < L2) {
            const tspgpu_city c = c2[t], d = c2[t + 1 == L2 ? 0 : t + 1];
            cx[t] = c.x, cy[t] = c.y, cid[t] = c.id;
            ce[t] = ddist(c.x, c.y, d.x, d.y);
        }
        __syncthreads();
        // one pass: the two smallest order keys of every swap cost (i over path
        // edges, j over block edges, pair index i * L2 + j = row-major order)
        Top2 tp{~0ull, ~0ull, ~0u};
        for (int i = t; i < len; i += kFoldThreads) {
            const int i1 = i + 1 == len ? 0 : i + 1;
            const double ax = px[i], ay = py[i], bx = px[i1], by = py[i1];
            const double eab = ddist(ax, ay, bx, by);
            for (int j = 0; j < L2; ++j) {
                const int j1 = j + 1 == L2 ? 0 : j + 1;
                const double sc = ((ddist(ax, ay, cx[j1], cy[j1]) + ddist(bx, by, cx[j], cy[j])) - eab) - ce[j];
                top2_add(tp, order_key(sc), (unsigned)(i * L2 + j));
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o *= 2) {
            Top2 q;
            q.k1 = shfl_u64(tp.k1, o);
            q.k2 = shfl_u64(tp.k2, o);
            q.i1 = (unsigned)__shfl_xor((int)tp.i1, o);
            tp = top2_merge(tp, q);
        }
        if (__lane_id() == 0) wtop[t / 64] = tp;
        __syncthreads();
        Top2 g = wtop[0];
#pragma unroll
        for (int w = 1; w < kFoldThreads / 64; ++w) g = top2_merge(g, wtop[w]);
        // exactly one pair within eps2 of the minimum (then it is the
        // reference's pair, as in fold_pick_kernel), else the host decides
        const double thr = key_value(g.k1) + eps2;
        if (!(g.k2 == ~0ull || g.k2 > order_key(thr))) {
            status = 1, at = m, nc = 2;
            break;
        }
        const int pi = (int)(g.i1 / (unsigned)L2), pj = (int)(g.i1 % (unsigned)L2);
        const int pi1 = pi + 1 == len ? 0 : pi + 1, pj1 = pj + 1 == L2 ? 0 : pj + 1;
        if (t == 0) {
            Cand k;
            k.i = pi, k.j = pj;
            k.a = tspgpu_city{pid[pi], px[pi], py[pi]};
            k.b = tspgpu_city{pid[pi1], px[pi1], py[pi1]};
            k.c = tspgpu_city{cid[pj], cx[pj], cy[pj]};
            k.d = tspgpu_city{cid[pj1], cx[pj1], cy[pj1]};
            J.picks[m].c = k;
        }
        // splice (tsp.cpp:240-259): p = first index of A or B in path 1 (0 when
        // either is its first city: the path closes on it), C's first index in
        // path 2 (0 for the closing copy); out = path[0..p] ++ reversed rotation
        // of the block after C ++ path[p+1..]
        const int first = pid[0];
        const int p = (pid[pi] == first || pid[pi1] == first) ? 0 : pi;
        const int sw = pj == L2 - 1 ? 0 : pj;
        const int start = (sw + 1) % M;
        // shift path[p+1 .. len) up by M: through registers (4 per thread at the cap)
        constexpr int kPer = kFoldCap / kFoldThreads;
        double sx[kPer], sy[kPer];
        int sid[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int k = p + 1 + t + q * kFoldThreads;
            if (k < len) sx[q] = px[k], sy[q] = py[k], sid[q] = pid[k];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int k = p + 1 + t + q * kFoldThreads;
            if (k < len) px[k + M] = sx[q], py[k + M] = sy[q], pid[k + M] = sid[q];
        }
        if (t < M) {
            const int k = p + 1 + t;
            const int q = start + (M - 1 - t);
            const int src = q >= M ? q - M : q;
            px[k] = cx[src], py[k] = cy[src], pid[k] = cid[src];
        }
        len += M;
    }
    __syncthreads();
    for (int k = t; k < len; k += kFoldThreads) J.path[k] = tspgpu_city{pid[k], px[k], py[k]};
    if (t == 0) {
        FoldOut o;
        o.status = status, o.at = at, o.len = len, o.count = nc;
        outs[blockIdx.x] = o;
    }
}

// ---- host side ---------------------------------------------------------------

double (*volatile g_pow)(double, double) = ::pow;
double (*volatile g_sqrt)(double) = ::sqrt;

double hdist(const tspgpu_city &a, const tspgpu_city &b)
{
    return g_sqrt(g_pow(a.x - b.x, 2) + g_pow(a.y - b.y, 2));  // assignment2.h:141-144
}

double hswap(const tspgpu_city &A, const tspgpu_city &B, const tspgpu_city &C, const tspgpu_city &D)
{
    return ((hdist(A, D) + hdist(B, C)) - hdist(A, B)) - hdist(C, D);  // tsp.cpp:197-200
}

// a path on the device: the buffer (capacity in cities) and the cities in use
struct DVec : DevBuf<tspgpu_city> {
    size_t len = 0;
    // grows only when nothing in flight references it (callers reserve up
    // front); the cities in use move to the new buffer
    int reserve(size_t n, hipStream_t st)
    {
        if (n <= cap) return 0;
        DevBuf<tspgpu_city> q;
        hipError_t e = tspgpu::dev_alloc(q, std::max<size_t>(n, cap * 2 + 64));
        if (e != hipSuccess) return hip_err(e);
        if (len) e = xcopy_async(q.p, p, len * sizeof(tspgpu_city), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        DevBuf<tspgpu_city>::operator=(std::move(q));
        return hip_err(e);
    }
};

// The merge stream.  merge() only enqueues: argmin, candidates, find, splice,
// all on the context's stream, no host round trip.  When exactly one pair is
// within eps2 of the device minimum it is the reference's pair (the exact
// minimum and all its ties are always inside the window) and the device
// splices at once; otherwise the stream stalls (later kernels return at once)
// and sync() lets the host pick with glibc pow, re-runs the stalled merge with
// the host's pair and re-enqueues the rest.  Costs, which need the exact swap
// cost (glibc pow) of every chosen pair, are folded on the host in merge order
// at sync(): cost_target = (cost_target + cost2) + best (tsp.cpp:263).
struct Merger {
    hipStream_t st = nullptr;
    int cus = 256;
    double eps2 = 0.0;
    DevBuf<Ctl> ctl;
    DevBuf<Cand> cand;
    DevBuf<Pick> picks;
    DevBuf<unsigned long long> blockmin;
    Pinned<Ctl> hctl;     // mirror of ctl
    Pinned<Pick> hpicks;  // mirror of picks
    struct Op {
        const tspgpu_city *src;
        tspgpu_city *dst;
        int L1;
        const tspgpu_city *c2;
        int L2;
        double *target;
        const double *cost2;
        bool fold;  // path 1 holds each city once + closing copy, path 2 is one block tour
    };
    std::vector<Op> ops;
    int init(tspgpu_ctx *c, double dmax)
    {
        st = c->stream;
        cus = c->cu_count;
        eps2 = 2.0 * std::ldexp(4.0 * dmax, -36);
        hipError_t e = tspgpu::dev_alloc(ctl, 1);
        if (e == hipSuccess) e = tspgpu::dev_alloc(cand, kCandCap);
        if (e == hipSuccess) e = tspgpu::dev_alloc(picks, kBatch);
        if (e == hipSuccess) e = tspgpu::dev_alloc(blockmin, kMaxBlocks);
        if (e == hipSuccess) e = tspgpu::pinned_alloc(hctl, 1);
        if (e == hipSuccess) e = tspgpu::pinned_alloc(hpicks, kBatch);
        if (e == hipSuccess) {
            Ctl z{};
            z.minkey = ~0ull;
            e = xcopy_async(ctl, &z, sizeof z, hipMemcpyHostToDevice, st);
        }
        ops.reserve(kBatch);
        return hip_err(e);
    }
    int grid_for(unsigned long long work) const
    {
        const unsigned long long b = (work + kMergeThreads - 1) / kMergeThreads;
        return (int)std::max<unsigned long long>(1, std::min<unsigned long long>(b, (unsigned long long)cus * 8));
    }
    // blockIdx.x strides path-1 edges, blockIdx.y path-2 chunks of *cw cities;
    // gx * gy <= kMaxBlocks.  The chunks narrow (down to 8 cities) until the
    // grid has about two blocks per CU: a tree merge of two ~1000-city paths
    // was 4 blocks on 4 CUs (argmin + candidates ~380 us, profiles/r05)
    dim3 pair_grid(int L1, int L2, int *cw) const
    {
        const int cap = std::min(cus * 8, kMaxBlocks);
        const int gx0 = std::max(1, std::min((L1 + kMergeThreads - 1) / kMergeThreads, cap));
        int w = kChunk;
        while (w > 8 && (long long)gx0 * ((L2 + w - 1) / w) < 2LL * cus) w /= 2;
        const int gy = std::min((L2 + w - 1) / w, cap);
        const int gx = std::max(1, std::min(gx0, cap / gy));
        *cw = w;
        return dim3(gx, gy);
    }
    void enqueue(const Op &o, int idx)
    {
        const int M = o.L2 - 1;
        if (o.fold && o.L2 <= kChunk) {
            const int gx = std::max(1, std::min((o.L1 + kMergeThreads - 1) / kMergeThreads, std::min(cus * 8, kMaxBlocks)));
            hipLaunchKernelGGL(fold_pick_kernel, dim3(gx), dim3(kMergeThreads), 0, st, o.src, o.L1, o.c2, o.L2, eps2,
                               ctl, blockmin, cand, picks, idx);
            hipLaunchKernelGGL(splice_kernel, dim3(grid_for(3ull * ((unsigned long long)o.L1 + M))),
                               dim3(kMergeThreads), 0, st, o.src, o.L1, o.c2, M, ctl, o.dst, idx, 0);
            return;
        }
        int cw = kChunk;
        const dim3 g = pair_grid(o.L1, o.L2, &cw);
        hipLaunchKernelGGL(argmin_kernel, g, dim3(kMergeThreads), 0, st, o.src, o.L1, o.c2, o.L2, cw, ctl, blockmin);
        hipLaunchKernelGGL(cand_kernel, g, dim3(kMergeThreads), 0, st, o.src, o.L1, o.c2, o.L2, cw, eps2, ctl, blockmin,
                           cand);
        hipLaunchKernelGGL(find_kernel, dim3(grid_for((unsigned long long)std::max(o.L1, M))), dim3(kMergeThreads), 0,
                           st, o.src, o.L1, o.c2, M, ctl, cand, picks, idx, 0, 0, 0, 0);
        hipLaunchKernelGGL(splice_kernel, dim3(grid_for(3ull * ((unsigned long long)o.L1 + M))), dim3(kMergeThreads),
                           0, st, o.src, o.L1, o.c2, M, ctl, o.dst, idx, 0);
    }
    // s1 <- mergeBlocks(s1, c2); *cost1 = (*cost1 + *cost2) + best once sync() ran.
    // tmp: a buffer of capacity >= s1.len + L2 - 1 (swapped with s1).
    int merge(DVec &s1, DVec &tmp, double *cost1, const tspgpu_city *c2, int L2, const double *cost2,
              bool fold = false)
    {
        const int L1 = (int)s1.len;
        if (L1 < 1 || L2 < 2) return -EINVAL;
        const int M = L2 - 1;
        if ((int)ops.size() == kBatch || tmp.cap < (size_t)L1 + M) {
            // (the reference's stale received lists can grow a path past all
            // cities: grow the spare buffer once nothing in flight uses it)
            int rc = sync();
            if (!rc) rc = tmp.reserve((size_t)L1 + M, st);
            if (rc) return rc;
        }
        Op o{s1.p, tmp.p, L1, c2, L2, cost1, cost2, fold};
        ops.push_back(o);
        enqueue(o, (int)ops.size() - 1);
        if (hipPeekAtLastError() != hipSuccess) return hip_err(hipGetLastError());
        std::swap(s1, tmp);
        s1.len = (size_t)L1 + M;
        tmp.len = 0;
        return 0;
    }
    // the host's pick for a stalled merge: exact (glibc) re-evaluation of the
    // candidates in row-major order with the reference's strict < from INT_MAX
    int host_pick(const Op &o, Cand &pick, double &best)
    {
        hipError_t e = hipSuccess;
        const unsigned long long nc = hctl->count;
        best = (double)INT_MAX;  // tsp.cpp:204
        bool found = false;
        if (nc > 0 && nc <= kCandCap) {
            std::vector<Cand> hc(nc);
            e = xcopy_async(hc.data(), cand, nc * sizeof(Cand), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_err(e);
            std::sort(hc.begin(), hc.end(),
                      [](const Cand &x, const Cand &y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
            for (const Cand &k : hc) {
                const double sc = hswap(k.a, k.b, k.c, k.d);
                if (sc < best) {
                    best = sc;
                    pick = k;
                    found = true;
                }
            }
        } else {
            // too many near-ties for the buffer: exact scan on the host
            std::vector<tspgpu_city> h1(o.L1), h2(o.L2);
            e = xcopy_async(h1.data(), o.src, o.L1 * sizeof(tspgpu_city), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = xcopy_async(h2.data(), o.c2, o.L2 * sizeof(tspgpu_city), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_err(e);
            for (int i = 0; i < o.L1; ++i)
                for (int j = 0; j < o.L2; ++j) {
                    const tspgpu_city &a = h1[i], &b = h1[(i + 1) % o.L1], &c = h2[j], &d = h2[(j + 1) % o.L2];
                    const double sc = hswap(a, b, c, d);
                    if (sc < best) {
                        best = sc;
                        pick = Cand{i, j, a, b, c, d};
                        found = true;
                    }
                }
        }
        return found ? 0 : -EIO;  // no swap below INT_MAX (distances are validated far below)
    }
    // run every enqueued merge to completion, resolving stalls on the host,
    // and fold their costs in order
    int sync()
    {
        size_t first = 0;  // ops[first..] not yet folded
        for (;;) {
            hipError_t e = xcopy_async(hctl, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_err(e);
            const size_t upto = hctl->stall ? (size_t)hctl->stall_at : ops.size();
            if (upto > first) {
                e = xcopy_async(hpicks + first, picks + first, (upto - first) * sizeof(Pick), hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st);
                if (e != hipSuccess) return hip_err(e);
                for (size_t m = first; m < upto; ++m) {
                    const Cand &k = hpicks[m].c;
                    *ops[m].target = (*ops[m].target + *ops[m].cost2) + hswap(k.a, k.b, k.c, k.d);
                }
                first = upto;
            }
            if (!hctl->stall) break;
            if (hctl->stall == 2) return -EDEADLK;
            if (hctl->stall != 1) return -EIO;
            // the host picks merge `first`, then the device splices it and the rest resumes
            const Op &o = ops[first];
            Cand pk{};
            double best = 0.0;
            int rc = host_pick(o, pk, best);
            if (rc) return rc;
            const int M = o.L2 - 1;
            Ctl reset = *hctl;
            reset.fw[0] = reset.fw[1] = ~0ull;
            e = xcopy_async(ctl, &reset, sizeof reset, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) return hip_err(e);
            hipLaunchKernelGGL(find_kernel, dim3(grid_for((unsigned long long)std::max(o.L1, M))),
                               dim3(kMergeThreads), 0, st, o.src, o.L1, o.c2, M, ctl, cand, picks, (int)first,
                               pk.a.id, pk.b.id, pk.c.id, 1);
            hipLaunchKernelGGL(splice_kernel, dim3(grid_for(3ull * ((unsigned long long)o.L1 + M))),
                               dim3(kMergeThreads), 0, st, o.src, o.L1, o.c2, M, ctl, o.dst, (int)first, 1);
            e = xcopy_async(hctl, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_err(e);
            if (hctl->stall == 2) return -EDEADLK;
            if (hctl->stall) return -EIO;
            *o.target = (*o.target + *o.cost2) + best;
            ++first;
            for (size_t m = first; m < ops.size(); ++m) enqueue(ops[m], (int)m);
            if (hipPeekAtLastError() != hipSuccess) return hip_err(hipGetLastError());
        }
        ops.clear();
        return 0;
    }
};

// mergeBlocks (tsp.cpp:202-269) on the host, exactly: glibc distances, first
// strict minimum in row-major order from INT_MAX, then the splice; for a fold
// merge that stalled the persistent kernel (several near-tied candidates).
// -> the pick (for the cost fold) and the new path in `path`.
int host_fold_merge(std::vector<tspgpu_city> &path, const tspgpu_city *c2, int L2, Cand &pick)
{
    const int L1 = (int)path.size(), M = L2 - 1;
    double best = (double)INT_MAX;  // tsp.cpp:204
    bool found = false;
    for (int i = 0; i < L1; ++i)
        for (int j = 0; j < L2; ++j) {
            const tspgpu_city &a = path[i], &b = path[(i + 1) % L1], &c = c2[j], &d = c2[(j + 1) % L2];
            const double sc = hswap(a, b, c, d);
            if (sc < best) {
                best = sc;
                pick = Cand{i, j, a, b, c, d};
                found = true;
            }
        }
    if (!found) return -EIO;
    // tsp.cpp:229-239: first index of A or B in path 1, of C in path 2 (without its closing copy)
    int p = -1, sw = -1;
    for (int k = 0; k < L1 && p < 0; ++k)
        if (path[k].id == pick.a.id || path[k].id == pick.b.id) p = k;
    for (int k = 0; k < M && sw < 0; ++k)
        if (c2[k].id == pick.c.id) sw = k;
    if (p < 0) return -EIO;
    if (sw < 0) return -EDEADLK;
    std::vector<tspgpu_city> out;
    out.reserve((size_t)L1 + M);
    const int start = (sw + 1) % M;
    for (int k = 0; k <= p; ++k) out.push_back(path[k]);
    for (int t = 0; t < M; ++t) {
        const int q = start + (M - 1 - t);
        out.push_back(c2[q >= M ? q - M : q]);
    }
    for (int k = p + 1; k < L1; ++k) out.push_back(path[k]);
    path.swap(out);
    return 0;
}

// The block paths the core reduces (DEVICE memory): nblocks paths of L cities
// each at p + b * L, or, with a descriptor table (block_desc.h; the same on
// the host and on the device), path b of desc[b].L cities at p + desc[b].path.
struct BlockSet {
    const tspgpu_city *p = nullptr;
    int nblocks = 0;
    int L = 0;                                   // every path's length (no table)
    const tspgpu::BlockDesc *h_desc = nullptr;   // host
    const tspgpu::BlockDesc *d_desc = nullptr;   // device
    size_t total = 0;                            // cities of all paths
    int max_len = 0;
    const tspgpu_city *at(int b) const { return p + (h_desc ? (size_t)h_desc[b].path : (size_t)b * L); }
    int len(int b) const { return h_desc ? h_desc[b].L : L; }
};
BlockSet uniform_blocks(const tspgpu_city *p, int L, int nblocks)
{
    BlockSet bs;
    bs.p = p, bs.nblocks = nblocks, bs.L = L, bs.total = (size_t)nblocks * L, bs.max_len = L;
    return bs;
}

// The fold of every logical rank (tsp.cpp:348-352) by fold_persist_kernel.
// Ranks that stall (several near-tied candidates) get the merge exactly on the
// host and are relaunched from the next one; ranks whose path outgrows LDS
// finish through the Merger's per-merge kernels.  rank[r] holds the path and
// rcost[r] the cost on return (costs folded in merge order, tsp.cpp:263, with
// glibc swap costs of the logged picks).
int persist_folds(Merger &m, const BlockSet &bs, const double *costs, const std::vector<int> &cnt,
                  std::vector<DVec> &rank, DVec &tmp, std::vector<double> &rcost)
{
    const int P = (int)cnt.size();
    int nb = 0;
    for (int c : cnt) nb += c;
    const size_t ncity = bs.total;
    const tspgpu_city *blocks = bs.p;
    DevBuf<FoldJob> djobs;
    DevBuf<FoldOut> douts;
    DevBuf<Pick> dpicks;
    hipError_t e = tspgpu::dev_alloc(djobs, P);
    if (e == hipSuccess) e = tspgpu::dev_alloc(douts, P);
    if (e == hipSuccess) e = tspgpu::dev_alloc(dpicks, (size_t)std::max(nb, 1));
    if (e != hipSuccess) return hip_err(e);
    std::vector<FoldJob> jobs(P);
    std::vector<int> firstb(P), cap_at(P, -1);
    std::vector<Pick> hpick((size_t)nb);
    std::vector<char> host_picked((size_t)nb, 0);
    int rc = 0;
    for (int r = 0, b = 0; r < P && !rc; b += cnt[r], ++r) {
        rc = rank[r].reserve(ncity, m.st);
        firstb[r] = b;
        jobs[r] = FoldJob{b, cnt[r], 0, 0, rank[r].p, dpicks + b};
    }
    std::vector<int> active(P);
    for (int r = 0; r < P; ++r) active[r] = r;
    std::vector<FoldOut> outs(P);
    while (!rc && !active.empty()) {
        std::vector<FoldJob> aj;
        for (int r : active) aj.push_back(jobs[r]);
        e = xcopy_async(djobs, aj.data(), aj.size() * sizeof(FoldJob), hipMemcpyHostToDevice, m.st);
        if (e == hipSuccess && bs.d_desc)
            hipLaunchKernelGGL(fold_persist_kernel<true>, dim3((unsigned)aj.size()), dim3(kFoldThreads), 0, m.st,
                               blocks, 0, bs.d_desc, m.eps2, djobs, douts);
        else if (e == hipSuccess)
            hipLaunchKernelGGL(fold_persist_kernel<false>, dim3((unsigned)aj.size()), dim3(kFoldThreads), 0, m.st,
                               blocks, bs.L, bs.d_desc, m.eps2, djobs, douts);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = xcopy_async(outs.data(), douts, aj.size() * sizeof(FoldOut), hipMemcpyDeviceToHost, m.st);
        if (e == hipSuccess) e = hipStreamSynchronize(m.st);
        if (e != hipSuccess) {
            rc = hip_err(e);
            break;
        }
        std::vector<int> again;
        for (size_t q = 0; q < active.size() && !rc; ++q) {
            const int r = active[q];
            const FoldOut &o = outs[q];
            rank[r].len = (size_t)o.len;
            if (o.status == 0) continue;
            if (o.status == 2) {  // the path outgrew LDS: the per-merge kernels take over at merge o.at
                cap_at[r] = o.at;
                continue;
            }
            // several candidates: merge o.at exactly on the host, then relaunch
            const int sb = firstb[r] + 1 + o.at, Lb = bs.len(sb);  // the stalled merge's block, its own length
            std::vector<tspgpu_city> path((size_t)o.len), blk((size_t)Lb);
            e = xcopy_async(path.data(), rank[r].p, path.size() * sizeof(tspgpu_city), hipMemcpyDeviceToHost, m.st);
            if (e == hipSuccess)
                e = xcopy_async(blk.data(), bs.at(sb), (size_t)Lb * sizeof(tspgpu_city), hipMemcpyDeviceToHost, m.st);
            if (e == hipSuccess) e = hipStreamSynchronize(m.st);
            if (e != hipSuccess) {
                rc = hip_err(e);
                break;
            }
            Cand pk{};
            rc = host_fold_merge(path, blk.data(), Lb, pk);
            if (rc) break;
            hpick[(size_t)firstb[r] + o.at].c = pk;
            host_picked[(size_t)firstb[r] + o.at] = 1;
            e = xcopy_async(rank[r].p, path.data(), path.size() * sizeof(tspgpu_city), hipMemcpyHostToDevice, m.st);
            if (e != hipSuccess) {
                rc = hip_err(e);
                break;
            }
            rank[r].len = path.size();
            jobs[r].k0 = o.at + 1;
            jobs[r].len = (int)path.size();
            if (jobs[r].k0 < cnt[r] - 1) again.push_back(r);
        }
        active.swap(again);
    }
    if (!rc) {
        // the logged picks -> exact costs in merge order (tsp.cpp:263)
        std::vector<Pick> dp((size_t)nb);
        e = xcopy_async(dp.data(), dpicks, dp.size() * sizeof(Pick), hipMemcpyDeviceToHost, m.st);
        if (e == hipSuccess) e = hipStreamSynchronize(m.st);
        rc = hip_err(e);
        for (int r = 0; r < P && !rc; ++r) {
            const int b0 = firstb[r];
            rcost[r] = costs[b0];
            const int done = cap_at[r] >= 0 ? cap_at[r] : cnt[r] - 1;
            for (int k = 0; k < done; ++k) {
                const size_t idx = (size_t)b0 + k;
                const Cand &c = host_picked[idx] ? hpick[idx].c : dp[idx].c;
                rcost[r] = (rcost[r] + costs[b0 + 1 + k]) + hswap(c.a, c.b, c.c, c.d);
            }
        }
        // the rest of an outgrown rank through the per-merge kernels
        for (int r = 0; r < P && !rc; ++r)
            for (int k = cap_at[r]; k >= 0 && k < cnt[r] - 1 && !rc; ++k)
                rc = m.merge(rank[r], tmp, &rcost[r], bs.at(firstb[r] + 1 + k), bs.len(firstb[r] + 1 + k),
                             &costs[firstb[r] + 1 + k], true);
    }
    if (!rc) rc = m.sync();  // (the picks buffer is freed on return: nothing in flight may use it)
    (void)hipStreamSynchronize(m.st);
    return rc;
}

double bbox_diagonal(const tspgpu_city *c, size_t n)
{
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (size_t i = 0; i < n; ++i) {
        x0 = std::min(x0, c[i].x);
        x1 = std::max(x1, c[i].x);
        y0 = std::min(y0, c[i].y);
        y1 = std::max(y1, c[i].y);
    }
    return tspgpu::path_bbox_diagonal(x0, x1, y0, y1);  // (shared with the device summary: paths_facts.h)
}

bool finite_cities(const tspgpu_city *c, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(c[i].x) || !std::isfinite(c[i].y)) return false;
    return true;
}

void put_log(const std::string &text, char *log, int logcap)
{
    if (!log || logcap <= 0) return;
    const size_t k = std::min(text.size(), (size_t)logcap - 1);
    std::memcpy(log, text.data(), k);
    log[k] = 0;
}

// Where the core leaves rank 0's final path: up to cap cities at p (a host
// or a device pointer; may be null with cap 0), the full length in *len.
struct PathDest {
    tspgpu_city *p;
    bool device;
    int cap;
    int *len;
};

// The core of the reduction (ctx->mu held, the device set): the distribution
// counts, every logical rank's left fold and the reduction tree over the
// block paths of `bs` (DEVICE memory: nblocks paths of one length or, with a
// descriptor table, of their own lengths; nblocks >= 2), costs on the host.  dmax: the cities' padded bounding-box diagonal;
// fold_ok: the paths close on their first city and ids are unique across
// blocks (the one-kernel fold merges' precondition).  -> *final_cost, the
// log text, and rank 0's final path into dest (optional).
int reduce_core(tspgpu_ctx *ctx, const BlockSet &bs, const double *costs, int nprocs, double dmax, bool fold_ok,
                double *final_cost, std::string &text, const PathDest *dest)
{
    const int nblocks = bs.nblocks;
    const size_t ncity = bs.total;
    Merger m;
    int rc = m.init(ctx, dmax);
    if (rc) return rc;
    // distributeBlocks' counts (tsp.cpp:167-192): rank r gets #{b in [1,B] : b mod P == r}
    std::vector<int> cnt(nprocs, 0);
    for (int b = nblocks; b > 0; --b) cnt[b % nprocs]++;
    // Every buffer a queued merge may touch is sized up front (a merged path
    // never exceeds all cities; a received list never exceeds all cities), so
    // nothing is reallocated while merges are in flight.
    std::vector<DVec> rank(nprocs), received(nprocs);
    DVec tmp;
    std::vector<double> rcost(nprocs, 0.0);
    rc = tmp.reserve(ncity, m.st);
    int next = 0;
    if (!rc && fold_ok && bs.max_len <= kFoldL2 && tspgpu::tuned_or("K3_PERSIST", 1) != 0) {
        // (tuning knob K3_PERSIST = 0: the per-merge launches instead; tests compare both)
        // every rank's fold in one persistent launch (fold_persist_kernel)
        rc = persist_folds(m, bs, costs, cnt, rank, tmp, rcost);
        next = nblocks;
    }
    for (int r = 0; r < nprocs && !rc && next < nblocks; ++r) {
        rc = rank[r].reserve(ncity, m.st);
        if (rc) break;
        rc = hip_err(xcopy_async(rank[r].p, bs.at(next), (size_t)bs.len(next) * sizeof(tspgpu_city),
                              hipMemcpyDeviceToDevice, m.st));
        rank[r].len = (size_t)bs.len(next);
        rcost[r] = costs[next];
        ++next;
        // each logical rank folds its contiguous block range left (tsp.cpp:348-352)
        for (int j = 1; j < cnt[r] && !rc; ++j, ++next)
            rc = m.merge(rank[r], tmp, &rcost[r], bs.at(next), bs.len(next), &costs[next], fold_ok);
    }
    // MPI_ManualReduce (tsp.cpp:52-134): the receiver appends every received
    // path to one function-local list and merges with the WHOLE list
    // (tsp.cpp:67,93-98,115-120)
    auto receive = [&](int to, int from) -> int {
        // the copy below reads rank[from]'s final path: every queued merge
        // (and any stall) must be resolved first
        int r2 = m.sync();
        if (r2) return r2;
        DVec &acc = received[to];
        const size_t add = rank[from].len;
        r2 = acc.reserve(std::max(acc.len + add, ncity), m.st);
        if (r2) return r2;
        r2 = hip_err(xcopy_async(acc.p + acc.len, rank[from].p, add * sizeof(tspgpu_city), hipMemcpyDeviceToDevice,
                                 m.st));
        if (r2) return r2;
        acc.len += add;
        return m.merge(rank[to], tmp, &rcost[to], acc.p, (int)acc.len, &rcost[from]);
    };
    const int lastpower = 1 << (int)std::log2((double)nprocs);
    for (int i = 0; i < nprocs - lastpower && !rc; ++i) {
        char line[128];
        std::snprintf(line, sizeof line, "process %i is about to receive %i cities from process %i\n", i,
                      (int)rank[i + lastpower].len, i + lastpower);  // tsp.cpp:88
        text += line;
        rc = receive(i, i + lastpower);
    }
    for (int d = 0; d < (int)std::log2((double)lastpower) && !rc; ++d)
        for (int k = 0; k < lastpower && !rc; k += 1 << (d + 1)) rc = receive(k, k + (1 << d));
    if (!rc) rc = m.sync();
    if (!rc && dest) {
        // rank 0 ends with finalSolution.path (tsp.cpp:355)
        *dest->len = (int)rank[0].len;
        const size_t k = std::min(rank[0].len, (size_t)dest->cap);
        if (k)
            rc = hip_err(xcopy_async(dest->p, rank[0].p, k * sizeof(tspgpu_city),
                                  dest->device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, m.st));
    }
    const hipError_t es = hipStreamSynchronize(m.st);
    if (!rc && dest) rc = hip_err(es);
    if (rc) return rc;
    *final_cost = rcost[0];
    return 0;
}

// The one-kernel fold merges need block tours that close on their first city
// and ids unique across blocks (the reference's generator numbers cities
// globally); anything else takes the general path.  The host scan.
// len: one length per path (concatenated paths), or null: L for every path.
bool host_fold_ok(const tspgpu_city *paths, int L, const int32_t *len, int nblocks)
{
    bool fold_ok = true;
    size_t total = 0;
    for (int b = 0; b < nblocks && fold_ok; ++b) {  // every path has at least 3 cities
        const int Lb = len ? len[b] : L;
        if (Lb < 3) fold_ok = false;
        total += (size_t)Lb;
    }
    if (fold_ok) {
        std::vector<int> ids;
        ids.reserve(total - (size_t)nblocks);
        const tspgpu_city *pb = paths;
        for (int b = 0; b < nblocks && fold_ok; ++b) {
            const int Lb = len ? len[b] : L;
            if (pb[0].id != pb[Lb - 1].id) fold_ok = false;
            for (int k = 0; k < Lb - 1; ++k) ids.push_back(pb[k].id);
            pb += Lb;
        }
        std::sort(ids.begin(), ids.end());
        if (fold_ok && std::adjacent_find(ids.begin(), ids.end()) != ids.end()) fold_ok = false;
    }
    return fold_ok;
}

// The descriptor table of concatenated paths (block_desc.h: path and L; city,
// dist and n are the caller's) on the host and, uploaded on st, on the device.
struct DescTable {
    std::vector<tspgpu::BlockDesc> h;
    DevBuf<tspgpu::BlockDesc> d;
    int upload(hipStream_t st)
    {
        if (hipError_t e = tspgpu::dev_alloc(d, h.size()); e != hipSuccess) return hip_err(e);
        // (an H2D copy has read the host table when it returns: xfer.h)
        return hip_err(xcopy_async(d, h.data(), h.size() * sizeof(tspgpu::BlockDesc), hipMemcpyHostToDevice, st));
    }
    BlockSet blocks(const tspgpu_city *p) const
    {
        BlockSet bs;
        bs.p = p, bs.nblocks = (int)h.size(), bs.h_desc = h.data(), bs.d_desc = d;
        for (const tspgpu::BlockDesc &e : h) {
            bs.total += (size_t)e.L;
            bs.max_len = std::max(bs.max_len, (int)e.L);
        }
        return bs;
    }
};

// The host front of tspgpu_reduce / tspgpu_reduce_path: argument checks, the
// three host scans, the upload, then the core.  dest null: no path wanted.
// len (tspgpu_reduce_ragged): the paths are concatenated and path b has len[b]
// cities; null: nblocks paths of L cities.
int reduce_host(tspgpu_ctx *ctx, const tspgpu_city *paths, int L, const int32_t *len, const double *costs, int nblocks,
                int nprocs, double *final_cost, const PathDest *dest, char *log, int logcap)
{
    if (log && logcap > 0) log[0] = 0;
    if (!ctx || !paths || !costs || !final_cost) return -EINVAL;
    if (nblocks < 1 || nprocs < 1 || nblocks < nprocs || (!len && L < 2)) return -EINVAL;
    if (dest && (!dest->len || dest->cap < 0 || (!dest->p && dest->cap > 0))) return -EINVAL;
    size_t ncity = (size_t)nblocks * L;
    DescTable table;
    if (len) {
        ncity = 0;
        for (int b = 0; b < nblocks; ++b) {
            if (len[b] < 2) return -EINVAL;
            ncity += (size_t)len[b];
        }
        if (ncity > (size_t)INT_MAX) return -EINVAL;  // (path lengths are ints throughout K3)
        table.h.resize((size_t)nblocks);
        int64_t at = 0;
        for (int b = 0; b < nblocks; ++b) {
            table.h[b] = tspgpu::BlockDesc{0, 0, at, 0, len[b]};
            at += len[b];
        }
        L = len[0];
    }
    if (!finite_cities(paths, ncity)) return -EINVAL;
    if (nblocks == 1) {  // one rank, one block: no fold, no tree (nothing to launch or load)
        *final_cost = costs[0];
        if (dest) {
            *dest->len = L;
            if (dest->cap > 0) std::memcpy(dest->p, paths, (size_t)std::min(L, dest->cap) * sizeof(tspgpu_city));
            if (dest->cap < L) return -ENOSPC;
        }
        return 0;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return -ENODEV;
    const double dmax = bbox_diagonal(paths, ncity);
    DVec blocks;
    int rc = blocks.reserve(ncity, ctx->stream);
    if (!rc) rc = hip_err(xcopy_async(blocks.p, paths, ncity * sizeof(tspgpu_city), hipMemcpyHostToDevice, ctx->stream));
    if (!rc) rc = hip_err(hipStreamSynchronize(ctx->stream));
    blocks.len = ncity;
    if (!rc && len) rc = table.upload(ctx->stream);
    std::string text;
    if (!rc)
        rc = reduce_core(ctx, len ? table.blocks(blocks.p) : uniform_blocks(blocks.p, L, nblocks), costs, nprocs, dmax,
                         host_fold_ok(paths, L, len, nblocks), final_cost, text, dest);
    if (rc) return rc;
    put_log(text, log, logcap);
    return dest && *dest->len > dest->cap ? -ENOSPC : 0;
}

}  // namespace

extern "C" {

int tspgpu_merge(tspgpu_ctx *ctx, const tspgpu_city *p1, int L1, double c1, const tspgpu_city *p2, int L2, double c2,
                 tspgpu_city *out, double *cost_out)
{
    if (!ctx || !p1 || !p2 || !out || !cost_out || L1 < 1 || L2 < 2) return -EINVAL;
    if (!finite_cities(p1, L1) || !finite_cities(p2, L2)) return -EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return -ENODEV;
    std::vector<tspgpu_city> all(p1, p1 + L1);
    all.insert(all.end(), p2, p2 + L2);
    Merger m;
    int rc = m.init(ctx, bbox_diagonal(all.data(), all.size()));
    DVec s, t, b;
    if (!rc) rc = s.reserve(L1, m.st);
    if (!rc) rc = t.reserve((size_t)L1 + L2, m.st);
    if (!rc) rc = b.reserve(L2, m.st);
    hipError_t e = hipSuccess;
    if (!rc) e = xcopy_async(s.p, p1, L1 * sizeof(tspgpu_city), hipMemcpyHostToDevice, m.st);
    if (!rc && e == hipSuccess) e = xcopy_async(b.p, p2, L2 * sizeof(tspgpu_city), hipMemcpyHostToDevice, m.st);
    if (!rc) rc = hip_err(e);
    s.len = L1;
    double cost = c1;
    if (!rc) rc = m.merge(s, t, &cost, b.p, L2, &c2);
    if (!rc) rc = m.sync();
    if (!rc) rc = hip_err(xcopy_async(out, s.p, s.len * sizeof(tspgpu_city), hipMemcpyDeviceToHost, m.st));
    if (!rc) rc = hip_err(hipStreamSynchronize(m.st));
    if (rc) return rc;
    *cost_out = cost;
    return (int)s.len;
}

int tspgpu_reduce(tspgpu_ctx *ctx, const tspgpu_city *paths, int L, const double *costs, int nblocks, int nprocs,
                  double *final_cost, char *log, int logcap)
{
    return reduce_host(ctx, paths, L, nullptr, costs, nblocks, nprocs, final_cost, nullptr, log, logcap);
}

int tspgpu_reduce_path(tspgpu_ctx *ctx, const tspgpu_city *paths, int L, const double *costs, int nblocks, int nprocs,
                       double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len, char *log, int logcap)
{
    if (!path_len) {
        if (log && logcap > 0) log[0] = 0;
        return -EINVAL;
    }
    const PathDest dest{path_out, false, path_cap, path_len};
    return reduce_host(ctx, paths, L, nullptr, costs, nblocks, nprocs, final_cost, &dest, log, logcap);
}

int tspgpu_reduce_ragged(tspgpu_ctx *ctx, const tspgpu_city *paths, const int32_t *len, const double *costs,
                         int nblocks, int nprocs, double *final_cost, tspgpu_city *path_out, int path_cap,
                         int *path_len, char *log, int logcap)
{
    if (!path_len || !len) {
        if (log && logcap > 0) log[0] = 0;
        return -EINVAL;
    }
    const PathDest dest{path_out, false, path_cap, path_len};
    return reduce_host(ctx, paths, 0, len, costs, nblocks, nprocs, final_cost, &dest, log, logcap);
}

}  // extern "C"

namespace {

// tspgpu_reduce_device (ns null: n cities and a tour row of n + 1 entries for
// every block) and tspgpu_reduce_ragged_device (ns: a host array, block b has
// ns[b] cities packed behind its predecessors', tour rows of tour_stride).
int reduce_device_front(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *d_tour, int tour_stride,
                        const double *d_cost, const int32_t *d_status, int n, const int32_t *ns, int nblocks,
                        int nprocs, double *final_cost, tspgpu_city *d_path_out, int path_cap, int *path_len,
                        char *log, int logcap, void *hip_stream)
{
    using tspgpu::PathFacts;
    if (log && logcap > 0) log[0] = 0;
    if (!ctx || !d_cities || !d_tour || !d_cost || !final_cost || !path_len) return -EINVAL;
    if (nblocks < 1 || nprocs < 1 || nblocks < nprocs) return -EINVAL;
    if (!ns && (n < 2 || n > TSPGPU_MAX_CITIES)) return -EINVAL;
    if (path_cap < 0 || (!d_path_out && path_cap > 0)) return -EINVAL;
    int L = ns ? 0 : tspgpu_tour_length(n), min_len = L;
    size_t ncity = (size_t)nblocks * L;
    DescTable table;
    if (ns) {
        // the packed layout is undefined unless every n[b] is in range
        int max_n = 0;
        ncity = 0;
        for (int b = 0; b < nblocks; ++b) {
            if (ns[b] < 2 || ns[b] > TSPGPU_MAX_CITIES) return -EINVAL;
            max_n = std::max(max_n, (int)ns[b]);
            ncity += (size_t)tspgpu_tour_length(ns[b]);
        }
        if (tour_stride < max_n + 1) return -EINVAL;
        table.h.resize((size_t)nblocks);
        int64_t city = 0, path = 0;
        min_len = INT_MAX;
        for (int b = 0; b < nblocks; ++b) {
            const int Lb = tspgpu_tour_length(ns[b]);
            table.h[b] = tspgpu::BlockDesc{city, 0, path, ns[b], Lb};
            city += ns[b];
            path += Lb;
            min_len = std::min(min_len, Lb);
        }
        L = table.h[0].L;  // (the one-block answer below)
    }
    if (ncity > (size_t)INT_MAX) return -EINVAL;  // (path lengths are ints throughout K3)
    std::lock_guard<std::mutex> g(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return -ENODEV;
    hipStream_t st = ctx->stream, caller = (hipStream_t)hip_stream;
    tspgpu::Event order;
    hipError_t e = hipSuccess;
    if (caller != st) {
        // K1's outputs were produced on the caller's stream
        e = hipEventCreateWithFlags(&order.p, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(order, caller);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, order, 0);
        if (e != hipSuccess) return hip_err(e);
    }
    // per call: the gathered paths, the facts, the id bitmap
    DVec blocks;
    DevBuf<PathFacts> d_facts;
    DevBuf<uint32_t> d_bitmap;
    // (whole words; for nblocks paths of L cities this is path_bitmap_bytes(nblocks, L))
    const size_t bitmap_bytes = (size_t)tspgpu::path_bitmap_bytes_total(ncity);
    int rc = blocks.reserve(ncity, st);
    if (!rc) rc = tspgpu::dev_reserve(d_facts, sizeof(PathFacts));
    if (!rc && min_len >= 3) rc = tspgpu::dev_reserve(d_bitmap, bitmap_bytes);
    if (!rc && ns) rc = table.upload(st);
    // (the timing events are the context's, created on the first call)
    if (!rc && !ctx->ev_k3_gather[0]) rc = hip_err(hipEventCreate(&ctx->ev_k3_gather[0].p));
    if (!rc && !ctx->ev_k3_gather[1]) rc = hip_err(hipEventCreate(&ctx->ev_k3_gather[1].p));
    PathFacts facts = tspgpu::path_facts_init();
    std::vector<double> costs((size_t)nblocks);
    const int grid_cap = ctx->cu_count * 8;
    if (!rc) rc = hip_err(xcopy_async(d_facts, &facts, sizeof facts, hipMemcpyHostToDevice, st));
    if (!rc && d_bitmap) rc = hip_err(hipMemsetAsync(d_bitmap, 0, bitmap_bytes, st));
    if (!rc) rc = hip_err(hipEventRecord(ctx->ev_k3_gather[0], st));
    if (!rc)
        rc = hip_err(ns ? tspgpu::launch_paths_gather_ragged(d_cities, d_tour, tour_stride, d_status, table.d, nblocks,
                                                          blocks.p, d_facts, grid_cap, st)
                     : tspgpu::launch_paths_gather(d_cities, d_tour, d_status, n, nblocks, blocks.p, d_facts, grid_cap,
                                                   st));
    if (!rc && d_bitmap)
        rc = hip_err(ns ? tspgpu::launch_paths_unique_ragged(blocks.p, table.d, nblocks, ncity, d_bitmap, d_facts,
                                                          grid_cap, st)
                     : tspgpu::launch_paths_unique(blocks.p, L, nblocks, d_bitmap, d_facts, grid_cap, st));
    if (!rc) rc = hip_err(hipEventRecord(ctx->ev_k3_gather[1], st));
    // (the D2H copies are complete when they return: xfer.h)
    if (!rc) rc = hip_err(xcopy_async(&facts, d_facts, sizeof facts, hipMemcpyDeviceToHost, st));
    if (!rc) rc = hip_err(xcopy_async(costs.data(), d_cost, costs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!rc) rc = hip_err(hipStreamSynchronize(st));
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    blocks.len = ncity;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ctx->ev_k3_gather[0], ctx->ev_k3_gather[1]) == hipSuccess) ctx->k3_gather_ms = ms;
    rc = tspgpu::path_facts_error(facts);
    std::string text;
    if (!rc && nblocks == 1) {  // one rank, one block: no fold, no tree
        *final_cost = costs[0];
        *path_len = L;
        const size_t k = (size_t)std::min(L, path_cap);
        if (k) rc = hip_err(xcopy_async(d_path_out, blocks.p, k * sizeof(tspgpu_city), hipMemcpyDeviceToDevice, st));
        if (!rc) rc = hip_err(hipStreamSynchronize(st));
    } else if (!rc) {
        // the host's own formula over the device's exact extrema: the bits of bbox_diagonal
        const double dmax = tspgpu::path_facts_diagonal(facts);
        const bool fold_ok = ns ? tspgpu::path_facts_fold_ok_ragged(facts, min_len) : tspgpu::path_facts_fold_ok(facts, L);
        const PathDest dest{d_path_out, true, path_cap, path_len};
        rc = reduce_core(ctx, ns ? table.blocks(blocks.p) : uniform_blocks(blocks.p, L, nblocks), costs.data(), nprocs,
                         dmax, fold_ok, final_cost, text, &dest);
    }
    if (rc) return rc;
    put_log(text, log, logcap);
    return *path_len > path_cap ? -ENOSPC : 0;
}

}  // namespace

extern "C" {

int tspgpu_reduce_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *d_tour, const double *d_cost,
                         const int32_t *d_status, int n, int nblocks, int nprocs, double *final_cost,
                         tspgpu_city *d_path_out, int path_cap, int *path_len, char *log, int logcap, void *hip_stream)
{
    return reduce_device_front(ctx, d_cities, d_tour, n + 1, d_cost, d_status, n, nullptr, nblocks, nprocs, final_cost,
                               d_path_out, path_cap, path_len, log, logcap, hip_stream);
}

int tspgpu_reduce_ragged_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *n, const int32_t *d_tour,
                                int tour_stride, const double *d_cost, const int32_t *d_status, int nblocks,
                                int nprocs, double *final_cost, tspgpu_city *d_path_out, int path_cap, int *path_len,
                                char *log, int logcap, void *hip_stream)
{
    if (!n) {
        if (log && logcap > 0) log[0] = 0;
        return -EINVAL;
    }
    return reduce_device_front(ctx, d_cities, d_tour, tour_stride, d_cost, d_status, 0, n, nblocks, nprocs, final_cost,
                               d_path_out, path_cap, path_len, log, logcap, hip_stream);
}

int tspgpu_reduce_device_last_ms(const tspgpu_ctx *ctx, double *gather_ms)
{
    if (!ctx) return -EINVAL;
    // (written by tspgpu_reduce_device under the context's mutex)
    std::lock_guard<std::mutex> g(const_cast<tspgpu_ctx *>(ctx)->mu);
    if (gather_ms) *gather_ms = ctx->k3_gather_ms;
    return 0;
}

}  // extern "C"

namespace {

// tspgpu_pipeline_cities (ns null: n cities in every block) and
// tspgpu_pipeline_cities_ragged (ns: packed blocks of ns[b] cities).  Per
// call: the cities, K1's outputs (tour rows of max n + 1 entries) and the
// merged tour on the device.  (Each step takes the context's mutex itself;
// the buffers are this call's.)
int pipeline_cities(tspgpu_ctx *ctx, const tspgpu_city *cities, int n, const int32_t *ns, bool ragged, int nblocks,
                    int nprocs, double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len, char *log,
                    int logcap)
{
    if (log && logcap > 0) log[0] = 0;
    if (!final_cost || !path_len || nblocks < 1 || nprocs < 1 || nblocks < nprocs) return -EINVAL;
    if (path_cap < 0 || (!path_out && path_cap > 0)) return -EINVAL;
    int max_n = 0;
    int64_t ncities = 0;
    if (tspgpu::cities_args(ctx, cities, n, ns, ragged, nblocks, 2, &max_n, &ncities)) return -EINVAL;
    const int stride = max_n + 1;
    // (every step below sets the same device, so it is still current when the
    // buffers free themselves on return)
    if (hipSetDevice(ctx->device) != hipSuccess) return -ENODEV;
    DevBuf<tspgpu_city> d_cities, d_path;
    DevBuf<double> d_cost;
    DevBuf<int32_t> d_tour, d_status;
    const size_t ib = (size_t)ncities * sizeof(tspgpu_city);
    int rc = tspgpu::dev_reserve(d_cities, ib);
    if (!rc) rc = tspgpu::dev_reserve(d_cost, (size_t)nblocks * sizeof(double));
    if (!rc) rc = tspgpu::dev_reserve(d_tour, (size_t)nblocks * stride * sizeof(int32_t));
    if (!rc) rc = tspgpu::dev_reserve(d_status, (size_t)nblocks * sizeof(int32_t));
    if (!rc && path_cap > 0) rc = tspgpu::dev_reserve(d_path, (size_t)path_cap * sizeof(tspgpu_city));
    void *st = tspgpu_stream(ctx);
    if (!rc) rc = tspgpu_memcpy_htod(ctx, d_cities, cities, ib);
    if (!rc)
        rc = ragged ? tspgpu_solve_cities_ragged_device(ctx, d_cities, ns, nblocks, d_cost, d_tour, stride, d_status, st)
                    : tspgpu_solve_cities_device(ctx, d_cities, n, nblocks, d_cost, d_tour, d_status, st);
    if (rc) {
        (void)tspgpu_stream_synchronize(ctx, st);
        return rc;
    }
    const int red = reduce_device_front(ctx, d_cities, d_tour, stride, d_cost, d_status, n, ns, nblocks, nprocs,
                                        final_cost, d_path, path_cap, path_len, log, logcap, st);
    if (red == 0 || red == -ENOSPC) {
        const size_t k = (size_t)std::min(*path_len, path_cap);
        if (k) rc = tspgpu_memcpy_dtoh(ctx, path_out, d_path, k * sizeof(tspgpu_city));
    }
    return rc ? rc : red;
}

}  // namespace

extern "C" {

int tspgpu_pipeline_cities(tspgpu_ctx *ctx, const tspgpu_city *cities, int n, int nblocks, int nprocs,
                           double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len, char *log,
                           int logcap)
{
    return pipeline_cities(ctx, cities, n, nullptr, false, nblocks, nprocs, final_cost, path_out, path_cap, path_len,
                           log, logcap);
}

int tspgpu_pipeline_cities_ragged(tspgpu_ctx *ctx, const tspgpu_city *cities, const int32_t *n, int nblocks,
                                  int nprocs, double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len,
                                  char *log, int logcap)
{
    return pipeline_cities(ctx, cities, 0, n, true, nblocks, nprocs, final_cost, path_out, path_cap, path_len, log,
                           logcap);
}

}  // extern "C"
