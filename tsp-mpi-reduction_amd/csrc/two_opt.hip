// 2-opt with a neighbour grid on a path (tspgpu_two_opt_path*):
// the kernels.  bounds validates and reduces the coordinates; cells, scan and
// fill build the grid once; search finds every position's best move under the
// order of the pass; apply performs the moves the host selected; emit gathers
// the input's cities into the final order.
//
// Exactness (the contract asks for the bits of the Python model): built with
// -ffp-contract=off, so every product, sum and quotient rounds where it is
// written; `/` on doubles is the correctly rounded division (the
// v_div_scale / v_div_fmas / v_div_fixup sequence, no fast-math flag); the
// square root is dist_exact.h's sqrt_rn, correctly rounded whatever the
// device's own sqrt rounds to.  Built without the K1 kernels' -fno-honor-nans:
// the bounds kernel must see a NaN coordinate.
//
// Indexing: L <= 2^30, so positions, cities, cells and slots are int32; the
// city arrays' 8-byte words (3 L) are indexed in 64 bits.
#include "two_opt.h"

#include "dist_exact.h"

namespace tspgpu {
namespace {

constexpr int kToThreads = 256;
constexpr int kToMaxGrid = 1 << 16;  // workgroups; longer arrays loop
constexpr int kScanPer = 4;          // items per lane of the first scan level
constexpr int kCityWords = 3;        // a city as 8-byte words: id + padding, x, y
static_assert(sizeof(tspgpu_city) == kCityWords * sizeof(uint64_t), "a city is three 8-byte words");

int to_grid(int64_t items)
{
    const int64_t wg = (items + kToThreads - 1) / kToThreads;
    return (int)(wg < 1 ? 1 : (wg < kToMaxGrid ? wg : kToMaxGrid));
}

// doubles as integers of the same order (-0.0 just below +0.0)
__host__ __device__ inline unsigned long long to_key(double v)
{
    const unsigned long long u = dist_bits(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline unsigned long long wave_min(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline unsigned long long wave_max(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One lane per city.  A wave reduces its keys with shuffles and its first
// lane issues the five integer atomics (at most 4 * kToMaxGrid waves).
__global__ __launch_bounds__(kToThreads) void two_opt_bounds_kernel(const tspgpu_city *__restrict__ path, int L,
                                                                   double *__restrict__ px, double *__restrict__ py,
                                                                   int32_t *__restrict__ ord,
                                                                   int32_t *__restrict__ pos,
                                                                   TwoOptBounds *__restrict__ bounds)
{
    unsigned long long xlo = ~0ull, xhi = 0ull, ylo = ~0ull, yhi = 0ull;
    int bad = 0;
    // (every lane of a wave takes the same number of turns: the shuffles below see whole waves)
    const int turns = (L + (int)gridDim.x * kToThreads - 1) / ((int)gridDim.x * kToThreads);
    for (int t = 0; t < turns; ++t) {
        const int64_t p64 = ((int64_t)t * gridDim.x + blockIdx.x) * kToThreads + threadIdx.x;
        if (p64 >= L) continue;
        const int p = (int)p64;
        const double x = path[p].x, y = path[p].y;
        px[p] = x;
        py[p] = y;
        ord[p] = p;
        pos[p] = p;
        if (isfinite(x) && isfinite(y)) {
            const unsigned long long kx = to_key(x), ky = to_key(y);
            xlo = kx < xlo ? kx : xlo;
            xhi = kx > xhi ? kx : xhi;
            ylo = ky < ylo ? ky : ylo;
            yhi = ky > yhi ? ky : yhi;
        } else {
            bad = 1;
        }
    }
    xlo = wave_min(xlo), ylo = wave_min(ylo), xhi = wave_max(xhi), yhi = wave_max(yhi);
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad != 0) != 0;
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&bounds->xmin, xlo);
        atomicMax(&bounds->xmax, xhi);
        atomicMin(&bounds->ymin, ylo);
        atomicMax(&bounds->ymax, yhi);
        if (any_bad) atomicOr(&bounds->nonfinite, 1ull);
    }
}

// the contract's cell index along one axis: IEEE division, then the product
__device__ inline int axis_cell(double v, double lo, double ext, int g)
{
    if (ext == 0.0) return 0;
    const int c = (int)(((v - lo) / ext) * (double)g);
    return c < 0 ? 0 : (c < g - 1 ? c : g - 1);  // (c >= 0 for validated input: v >= lo)
}

__global__ __launch_bounds__(kToThreads) void two_opt_cells_kernel(const double *__restrict__ x,
                                                                  const double *__restrict__ y, int L, double xmin,
                                                                  double ex, double ymin, double ey, int g,
                                                                  int32_t *__restrict__ cell,
                                                                  int32_t *__restrict__ count)
{
    for (int64_t p = (int64_t)blockIdx.x * kToThreads + threadIdx.x; p < L; p += (int64_t)gridDim.x * kToThreads) {
        const int c = axis_cell(y[p], ymin, ey, g) * g + axis_cell(x[p], xmin, ex, g);
        cell[p] = c;
        atomicAdd(&count[c], 1);
    }
}

// One level of the exclusive scan: a workgroup covers kToThreads * per
// consecutive items, a lane `per` of them; out[k] = the sum of the items
// before k inside the workgroup's span, sums[blockIdx] its total (when asked
// for).  in == out is allowed: a lane reads an item before it writes there,
// and no lane touches another's items.
__global__ __launch_bounds__(kToThreads) void two_opt_scan_kernel(const int32_t *in, int n, int per, int32_t *out,
                                                                 int32_t *sums)
{
    __shared__ int32_t sh[kToThreads];
    const int t = threadIdx.x;
    const int64_t base = ((int64_t)blockIdx.x * kToThreads + t) * per;
    int32_t mine = 0;
    for (int k = 0; k < per; ++k)
        if (base + k < n) mine += in[base + k];
    sh[t] = mine;
    __syncthreads();
    for (int off = 1; off < kToThreads; off <<= 1) {
        const int32_t v = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    int32_t run = sh[t] - mine;
    if (sums && t == kToThreads - 1) sums[blockIdx.x] = sh[t];
    for (int k = 0; k < per; ++k)
        if (base + k < n) {
            const int32_t v = in[base + k];
            out[base + k] = run;
            run += v;
        }
}

// start[k] += the scanned total of the workgroups before k's; start[n] = total
__global__ __launch_bounds__(kToThreads) void two_opt_scan_add_kernel(int32_t *__restrict__ start, int n, int span,
                                                                     const int32_t *__restrict__ sums, int32_t total)
{
    for (int64_t k = (int64_t)blockIdx.x * kToThreads + threadIdx.x; k <= n; k += (int64_t)gridDim.x * kToThreads)
        start[k] = k < n ? start[k] + sums[k / span] : total;
}

__global__ __launch_bounds__(kToThreads) void two_opt_fill_kernel(const double *__restrict__ x,
                                                                 const double *__restrict__ y,
                                                                 const int32_t *__restrict__ cell, int L,
                                                                 const int32_t *__restrict__ start,
                                                                 int32_t *__restrict__ cursor,
                                                                 double *__restrict__ cell_x,
                                                                 double *__restrict__ cell_y,
                                                                 int32_t *__restrict__ cell_city)
{
    for (int64_t p = (int64_t)blockIdx.x * kToThreads + threadIdx.x; p < L; p += (int64_t)gridDim.x * kToThreads) {
        const int c = cell[p];
        const int slot = start[c] + atomicAdd(&cursor[c], 1);
        if (slot < 0 || slot >= L) continue;  // (cannot happen while count, start and cursor agree)
        cell_x[slot] = x[p];
        cell_y[slot] = y[p];
        cell_city[slot] = (int32_t)p;
    }
}

__device__ inline double to_dist(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx, dy = ay - by;
    return sqrt_rn(dx * dx + dy * dy);
}

// The running best of one position: the largest gain > 0, the smallest j on
// equal gains.  A j that both forms reach computes the same gain from the
// same operands twice, so it cannot displace itself.
struct ToBest {
    double gain = 0.0;
    int j = -1;
    __device__ void offer(double g, int jj)
    {
        if (g > gain || (g == gain && j >= 0 && jj < j)) gain = g, j = jj;
    }
};

// One lane per position i (a = ord[i], b = ord[i+1]).  The cells within
// `ring` of a city's cell are, row by row, consecutive cells, so one row is
// one contiguous run of the cell-sorted arrays: start[row * g + x0] up to
// start[row * g + x1 + 1].  Successor form (`pred` 0): the listed city is c at
// j = pos[c], its coordinates come from the run, e's from px/py[j+1].
// Predecessor form: the listed city is e at j + 1 = pos[e], c's come from
// px/py[j].
template <int pred>
__device__ inline void to_walk(int centre, int i, int L, int g, int ring, double ax, double ay, double bx, double by,
                               double dab, const int32_t *__restrict__ pos, const double *__restrict__ px,
                               const double *__restrict__ py, const int32_t *__restrict__ start,
                               const double *__restrict__ cell_x, const double *__restrict__ cell_y,
                               const int32_t *__restrict__ cell_city, ToBest &best)
{
    const int ccx = centre % g, ccy = centre / g;
    const int x0 = ccx - ring < 0 ? 0 : ccx - ring, x1 = ccx + ring > g - 1 ? g - 1 : ccx + ring;
    const int y0 = ccy - ring < 0 ? 0 : ccy - ring, y1 = ccy + ring > g - 1 ? g - 1 : ccy + ring;
    for (int row = y0; row <= y1; ++row) {
        const int s = start[row * g + x0], e = start[row * g + x1 + 1];
        for (int k = s; k < e; ++k) {
            const int j = pos[cell_city[k]] - pred;
            if (j < i + 2 || j > L - 2) continue;
            const double lx = cell_x[k], ly = cell_y[k];
            double cx, cy, ex, ey;
            if (pred) {
                cx = px[j], cy = py[j], ex = lx, ey = ly;
            } else {
                cx = lx, cy = ly, ex = px[j + 1], ey = py[j + 1];
            }
            const double gain = (dab + to_dist(cx, cy, ex, ey)) - (to_dist(ax, ay, cx, cy) + to_dist(bx, by, ex, ey));
            best.offer(gain, j);
        }
    }
}

__global__ __launch_bounds__(kToThreads) void two_opt_search_kernel(
    int L, int g, int ring, const int32_t *__restrict__ ord, const int32_t *__restrict__ pos,
    const double *__restrict__ px, const double *__restrict__ py, const int32_t *__restrict__ cell,
    const int32_t *__restrict__ start, const double *__restrict__ cell_x, const double *__restrict__ cell_y,
    const int32_t *__restrict__ cell_city, TwoOptCand *__restrict__ cand, uint32_t *__restrict__ count)
{
    // i <= L - 4: the first legal j is i + 2 <= L - 2
    for (int64_t i64 = (int64_t)blockIdx.x * kToThreads + threadIdx.x; i64 <= (int64_t)L - 4;
         i64 += (int64_t)gridDim.x * kToThreads) {
        const int i = (int)i64;
        const double ax = px[i], ay = py[i], bx = px[i + 1], by = py[i + 1];
        const double dab = to_dist(ax, ay, bx, by);
        ToBest best;
        to_walk<0>(cell[ord[i]], i, L, g, ring, ax, ay, bx, by, dab, pos, px, py, start, cell_x, cell_y, cell_city,
                   best);
        to_walk<1>(cell[ord[i + 1]], i, L, g, ring, ax, ay, bx, by, dab, pos, px, py, start, cell_x, cell_y,
                   cell_city, best);
        if (best.j >= 0) {
            const uint32_t slot = atomicAdd(count, 1u);
            if (slot < (uint32_t)L) cand[slot] = TwoOptCand{best.gain, i, best.j};  // (one per position: below L)
        }
    }
}

// One lane per swap.  Swap t belongs to the move m with prefix[m] <= t <
// prefix[m+1] and exchanges positions i+1+r and j-r, r = t - prefix[m]; the
// moves' ranges are disjoint, so no two lanes touch one position.
__global__ __launch_bounds__(kToThreads) void two_opt_apply_kernel(int moves, const int32_t *__restrict__ acc_i,
                                                                  const int32_t *__restrict__ acc_j,
                                                                  const int32_t *__restrict__ prefix, int swaps,
                                                                  int32_t *__restrict__ ord,
                                                                  int32_t *__restrict__ pos, double *__restrict__ px,
                                                                  double *__restrict__ py)
{
    for (int64_t t64 = (int64_t)blockIdx.x * kToThreads + threadIdx.x; t64 < swaps;
         t64 += (int64_t)gridDim.x * kToThreads) {
        const int t = (int)t64;
        int lo = 0, hi = moves - 1;  // the last m with prefix[m] <= t
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (prefix[mid] <= t)
                lo = mid;
            else
                hi = mid - 1;
        }
        const int r = t - prefix[lo];
        const int k = acc_i[lo] + 1 + r, k2 = acc_j[lo] - r;
        const int ck = ord[k], ck2 = ord[k2];
        const double xk = px[k], yk = py[k], xk2 = px[k2], yk2 = py[k2];
        ord[k] = ck2, ord[k2] = ck;
        pos[ck2] = k, pos[ck] = k2;
        px[k] = xk2, py[k] = yk2;
        px[k2] = xk, py[k2] = yk;
    }
}

// one 8-byte word per lane, the output written in order
__global__ __launch_bounds__(kToThreads) void two_opt_emit_kernel(const uint64_t *__restrict__ in,
                                                                 const int32_t *__restrict__ ord, int L,
                                                                 uint64_t *__restrict__ out)
{
    const int64_t total = (int64_t)L * kCityWords;
    for (int64_t w = (int64_t)blockIdx.x * kToThreads + threadIdx.x; w < total;
         w += (int64_t)gridDim.x * kToThreads) {
        const int64_t p = w / kCityWords;
        out[w] = in[(int64_t)ord[p] * kCityWords + (w - p * kCityWords)];
    }
}

}  // namespace

TwoOptBounds two_opt_bounds_init() { return TwoOptBounds{~0ull, 0ull, ~0ull, 0ull, 0ull}; }

double two_opt_decode(unsigned long long key)
{
    return dist_from_bits((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key);
}

hipError_t launch_two_opt_bounds(const tspgpu_city *path, int L, double *px, double *py, int32_t *ord, int32_t *pos,
                                 TwoOptBounds *bounds, hipStream_t stream)
{
    if (L < 1) return hipErrorInvalidValue;
    void *args[] = {&path, &L, &px, &py, &ord, &pos, &bounds};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_bounds_kernel), dim3(to_grid(L)),
                           dim3(kToThreads), args, 0, stream);
}

hipError_t launch_two_opt_cells(const double *x, const double *y, int L, double xmin, double ex, double ymin,
                                double ey, int g, int32_t *cell, int32_t *count, hipStream_t stream)
{
    if (L < 1 || g < 1 || g > kTwoOptMaxGrid) return hipErrorInvalidValue;
    void *args[] = {&x, &y, &L, &xmin, &ex, &ymin, &ey, &g, &cell, &count};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_cells_kernel), dim3(to_grid(L)), dim3(kToThreads),
                           args, 0, stream);
}

hipError_t launch_two_opt_scan(const int32_t *count, int cells, int32_t total, int32_t *start, int32_t *sums,
                               hipStream_t stream)
{
    if (cells < 1 || cells > kTwoOptMaxGrid * kTwoOptMaxGrid) return hipErrorInvalidValue;
    int span = kToThreads * kScanPer;
    int nb = (cells + span - 1) / span;  // <= 4096: the second level is one workgroup
    int per = kScanPer, per2 = (nb + kToThreads - 1) / kToThreads;
    int32_t *none = nullptr;
    void *a1[] = {&count, &cells, &per, &start, &sums};
    hipError_t e = hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_scan_kernel), dim3(nb), dim3(kToThreads),
                                   a1, 0, stream);
    if (e != hipSuccess) return e;
    void *a2[] = {&sums, &nb, &per2, &sums, &none};
    e = hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_scan_kernel), dim3(1), dim3(kToThreads), a2, 0,
                        stream);
    if (e != hipSuccess) return e;
    void *a3[] = {&start, &cells, &span, &sums, &total};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_scan_add_kernel), dim3(to_grid((int64_t)cells + 1)),
                           dim3(kToThreads), a3, 0, stream);
}

hipError_t launch_two_opt_fill(const double *x, const double *y, const int32_t *cell, int L, const int32_t *start,
                               int32_t *cursor, double *cell_x, double *cell_y, int32_t *cell_city,
                               hipStream_t stream)
{
    if (L < 1) return hipErrorInvalidValue;
    void *args[] = {&x, &y, &cell, &L, &start, &cursor, &cell_x, &cell_y, &cell_city};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_fill_kernel), dim3(to_grid(L)), dim3(kToThreads),
                           args, 0, stream);
}

hipError_t launch_two_opt_search(int L, int g, int ring, const int32_t *ord, const int32_t *pos, const double *px,
                                 const double *py, const int32_t *cell, const int32_t *start, const double *cell_x,
                                 const double *cell_y, const int32_t *cell_city, TwoOptCand *cand, uint32_t *count,
                                 hipStream_t stream)
{
    if (L < 4 || g < 1 || g > kTwoOptMaxGrid || ring < 1 || ring > kTwoOptMaxRing) return hipErrorInvalidValue;
    void *args[] = {&L, &g, &ring, &ord, &pos, &px, &py, &cell, &start, &cell_x, &cell_y, &cell_city, &cand, &count};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_search_kernel), dim3(to_grid((int64_t)L - 3)),
                           dim3(kToThreads), args, 0, stream);
}

hipError_t launch_two_opt_apply(int moves, const int32_t *acc_i, const int32_t *acc_j, const int32_t *prefix, int swaps,
                                int32_t *ord, int32_t *pos, double *px, double *py, hipStream_t stream)
{
    if (moves <= 0 || swaps <= 0) return hipSuccess;
    void *args[] = {&moves, &acc_i, &acc_j, &prefix, &swaps, &ord, &pos, &px, &py};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_apply_kernel), dim3(to_grid(swaps)),
                           dim3(kToThreads), args, 0, stream);
}

hipError_t launch_two_opt_emit(const tspgpu_city *in, const int32_t *ord, int L, tspgpu_city *out, hipStream_t stream)
{
    if (L < 1) return hipErrorInvalidValue;
    const uint64_t *s = reinterpret_cast<const uint64_t *>(in);
    uint64_t *d = reinterpret_cast<uint64_t *>(out);
    void *args[] = {&s, &ord, &L, &d};
    return hipLaunchKernel(reinterpret_cast<const void *>(&two_opt_emit_kernel),
                           dim3(to_grid((int64_t)L * kCityWords)), dim3(kToThreads), args, 0, stream);
}

}  // namespace tspgpu
