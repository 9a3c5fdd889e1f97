// Or-opt with a neighbour grid on a path (tspgpu_or_opt_path*):
// the kernels that are not the 2-opt stage's.  search finds every position's
// best segment insertion under the order of the pass; stage and commit perform
// the rotations the host selected.  Bounds, grid and emit are two_opt.hip's.
//
// Exactness as in two_opt.hip: -ffp-contract=off, NaNs honoured (a segment
// that does not fit carries a NaN and so never compares greater), sqrt_rn.
//
// Indexing: L <= 2^30, so positions, cities, slots and the flat index over the
// rotated ranges (their lengths sum to less than L) are int32.
#include "or_opt.h"

#include "dist_exact.h"

namespace tspgpu {
namespace {

constexpr int kOoThreads = 256;
constexpr int kOoMaxGrid = 1 << 16;  // workgroups; longer arrays loop

int oo_grid(int64_t items)
{
    const int64_t wg = (items + kOoThreads - 1) / kOoThreads;
    return (int)(wg < 1 ? 1 : (wg < kOoMaxGrid ? wg : kOoMaxGrid));
}

__device__ inline double oo_dist(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx, dy = ay - by;
    return sqrt_rn(dx * dx + dy * dy);
}

// (a, k, t, rev) as one integer of the same lexicographic order: a and t are
// below 2^30, k below 4
__device__ inline unsigned long long oo_key(int a, int k, int t, int rev)
{
    return ((unsigned long long)a << 33) | ((unsigned long long)k << 31) | ((unsigned long long)t << 1) |
           (unsigned long long)rev;
}

// The running best of one position: the largest gain > 0, the smallest tuple
// on equal gains.  A move reached twice computes the same gain from the same
// operands, so it cannot displace itself.
struct OoBest {
    double gain = 0.0;
    unsigned long long key = ~0ull;
    __device__ void offer(double g, unsigned long long kk)
    {
        if (g > gain || (g == gain && gain > 0.0 && kk < key)) gain = g, key = kk;
    }
};

// One lane per position s (f = ord[s]).  SEG = max_seg.  The lane's segments,
// 2 SEG - 1 of them: n = 0 is f alone; n = 1 .. SEG-1 has f first (k = n + 1
// positions s .. s+k-1); n = SEG .. 2 SEG-2 has f last (k = n - SEG + 2
// positions s-k+1 .. s).  For each the lane keeps the other end's coordinates
// (w[] below), rem = d(P,first) + d(last,N) and d(P,N); a segment that does
// not fit inside 1 .. L-2 keeps rem = NaN, which makes each of its gains a NaN.
//
// Per listed neighbour v at q = pos[v]: v's coordinates from the run, those of
// positions q-1 and q+1 from px/py, d(f,v), d(v,p[q-1]) and d(v,p[q+1]) once,
// then per segment the insertion into edge q (c = v; f follows it, the other
// end meets p[q+1]) and into edge q-1 (e = v; f precedes it, the other end
// meets p[q-1]): one more distance each.
template <int SEG>
__global__ __launch_bounds__(kOoThreads) void or_opt_search_kernel(
    int L, int g, int ring, const int32_t *__restrict__ ord, const int32_t *__restrict__ pos,
    const double *__restrict__ px, const double *__restrict__ py, const int32_t *__restrict__ cell,
    const int32_t *__restrict__ start, const double *__restrict__ cell_x, const double *__restrict__ cell_y,
    const int32_t *__restrict__ cell_city, OrOptCand *__restrict__ cand, uint32_t *__restrict__ count)
{
    constexpr int NS = 2 * SEG - 1;
    for (int64_t s64 = (int64_t)blockIdx.x * kOoThreads + threadIdx.x + 1; s64 <= (int64_t)L - 2;
         s64 += (int64_t)gridDim.x * kOoThreads) {
        const int s = (int)s64;
        // positions s-SEG .. s+SEG, clamped into the path (a clamped one belongs to a segment that does not fit)
        double wx[2 * SEG + 1], wy[2 * SEG + 1];
#pragma unroll
        for (int d = -SEG; d <= SEG; ++d) {
            const int p = s + d < 0 ? 0 : (s + d > L - 1 ? L - 1 : s + d);
            wx[d + SEG] = px[p], wy[d + SEG] = py[p];
        }
        const double fx = wx[SEG], fy = wy[SEG];
        double rem[NS], dpn[NS];
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const bool lead = n < SEG;
            const int k = lead ? n + 1 : n - SEG + 2;
            const int a = lead ? 0 : -(k - 1), h = a + k - 1;  // relative to s
            const bool fits = s + a >= 1 && s + h <= L - 2;
            const double Px = wx[a - 1 + SEG], Py = wy[a - 1 + SEG], Nx = wx[h + 1 + SEG], Ny = wy[h + 1 + SEG];
            const double r = oo_dist(Px, Py, wx[a + SEG], wy[a + SEG]) + oo_dist(wx[h + SEG], wy[h + SEG], Nx, Ny);
            rem[n] = fits ? r : __builtin_nan("");
            dpn[n] = oo_dist(Px, Py, Nx, Ny);
        }
        OoBest best;
        const int centre = cell[ord[s]];
        const int ccx = centre % g, ccy = centre / g;
        const int x0 = ccx - ring < 0 ? 0 : ccx - ring, x1 = ccx + ring > g - 1 ? g - 1 : ccx + ring;
        const int y0 = ccy - ring < 0 ? 0 : ccy - ring, y1 = ccy + ring > g - 1 ? g - 1 : ccy + ring;
        for (int row = y0; row <= y1; ++row) {
            const int from = start[row * g + x0], to = start[row * g + x1 + 1];
            for (int slot = from; slot < to; ++slot) {
                const int q = pos[cell_city[slot]];
                if (q == s) continue;  // v = f
                const double vx = cell_x[slot], vy = cell_y[slot];
                const double dfv = oo_dist(fx, fy, vx, vy);
                if (q <= L - 2) {  // t = q: c = v, e = p[q+1]
                    const double ex = px[q + 1], ey = py[q + 1];
                    const double dce = oo_dist(vx, vy, ex, ey);
#pragma unroll
                    for (int n = 0; n < NS; ++n) {
                        const bool lead = n < SEG;
                        const int k = lead ? n + 1 : n - SEG + 2;
                        const int far = lead ? k - 1 : -(k - 1);  // y, the end that is not f
                        const int a = lead ? s : s - (k - 1), h = a + k - 1;
                        if (q >= a - 1 && q <= h) continue;
                        const double gain =
                            (rem[n] + dce) - ((dpn[n] + dfv) + oo_dist(wx[far + SEG], wy[far + SEG], ex, ey));
                        best.offer(gain, oo_key(a, k, q, lead ? 0 : 1));
                    }
                }
                if (q >= 1) {  // t = q - 1: c = p[q-1], e = v
                    const double cx = px[q - 1], cy = py[q - 1];
                    const double dce = oo_dist(vx, vy, cx, cy);
#pragma unroll
                    for (int n = 0; n < NS; ++n) {
                        const bool lead = n < SEG;
                        const int k = lead ? n + 1 : n - SEG + 2;
                        const int far = lead ? k - 1 : -(k - 1);  // x, the end that is not f
                        const int a = lead ? s : s - (k - 1), h = a + k - 1;
                        if (q - 1 >= a - 1 && q - 1 <= h) continue;
                        const double gain =
                            (rem[n] + dce) - ((dpn[n] + oo_dist(cx, cy, wx[far + SEG], wy[far + SEG])) + dfv);
                        best.offer(gain, oo_key(a, k, q - 1, lead && k > 1 ? 1 : 0));
                    }
                }
            }
        }
        if (best.key != ~0ull) {
            const uint32_t slot = atomicAdd(count, 1u);
            if (slot < (uint32_t)L)  // (one per position: below L)
                cand[slot] = OrOptCand{best.gain, s, (int32_t)(best.key >> 33),
                                       (int32_t)((best.key >> 1) & 0x3fffffffu),
                                       or_opt_kr((int)((best.key >> 31) & 3u), (int)(best.key & 1u))};
        }
    }
}

// the move a flat index belongs to: the last m with prefix[m] <= r
__device__ inline int oo_move_of(int r, int moves, const int32_t *__restrict__ prefix)
{
    int lo = 0, hi = moves - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// One lane per rotated position.  Flat index r belongs to move m and to
// position lo+1+j, j = r - prefix[m]; its new city is the old one of `src`:
// with n = hi - lo positions and a segment of k, a forward move puts the
// n - k others first and the segment last, a backward move the segment first.
// stage reads the state and writes scratch only, commit reads scratch only:
// the new values of a range depend on old ones elsewhere in the same range.
__global__ __launch_bounds__(kOoThreads) void or_opt_stage_kernel(
    int moves, const int32_t *__restrict__ acc_lo, const int32_t *__restrict__ acc_hi,
    const int32_t *__restrict__ acc_how, const int32_t *__restrict__ prefix, int total,
    const int32_t *__restrict__ ord, const double *__restrict__ px, const double *__restrict__ py,
    int32_t *__restrict__ s_ord, double *__restrict__ s_x, double *__restrict__ s_y)
{
    for (int64_t r64 = (int64_t)blockIdx.x * kOoThreads + threadIdx.x; r64 < total;
         r64 += (int64_t)gridDim.x * kOoThreads) {
        const int r = (int)r64;
        const int m = oo_move_of(r, moves, prefix);
        const int j = r - prefix[m], lo = acc_lo[m], hi = acc_hi[m], how = acc_how[m];
        const int n = hi - lo, k = how & 3;
        const bool rev = (how & 4) != 0, fwd = (how & kOrOptFwd) != 0;
        int src;
        if (fwd) {  // the segment is lo+1 .. lo+k
            const int i = j - (n - k);
            src = i < 0 ? lo + 1 + k + j : (rev ? lo + k - i : lo + 1 + i);
        } else {  // the segment is hi-k+1 .. hi
            src = j < k ? (rev ? hi - j : hi - k + 1 + j) : lo + 1 + (j - k);
        }
        if (k < 1 || k >= n || src <= lo || src > hi) continue;  // (cannot happen for a selected move)
        s_ord[r] = ord[src];
        s_x[r] = px[src];
        s_y[r] = py[src];
    }
}

__global__ __launch_bounds__(kOoThreads) void or_opt_commit_kernel(
    int moves, const int32_t *__restrict__ acc_lo, const int32_t *__restrict__ acc_hi,
    const int32_t *__restrict__ acc_how, const int32_t *__restrict__ prefix, int total, int L,
    const int32_t *__restrict__ s_ord, const double *__restrict__ s_x, const double *__restrict__ s_y,
    int32_t *__restrict__ ord, int32_t *__restrict__ pos, double *__restrict__ px, double *__restrict__ py)
{
    for (int64_t r64 = (int64_t)blockIdx.x * kOoThreads + threadIdx.x; r64 < total;
         r64 += (int64_t)gridDim.x * kOoThreads) {
        const int r = (int)r64;
        const int m = oo_move_of(r, moves, prefix);
        const int lo = acc_lo[m], hi = acc_hi[m], k = acc_how[m] & 3;
        const int w = lo + 1 + (r - prefix[m]);
        const int city = s_ord[r];
        if (k < 1 || k >= hi - lo || w <= lo || w > hi || w >= L || city < 0 || city >= L) continue;  // (as in stage)
        ord[w] = city;
        pos[city] = w;
        px[w] = s_x[r];
        py[w] = s_y[r];
    }
}

template <int SEG>
hipError_t oo_search(int L, int g, int ring, const int32_t *ord, const int32_t *pos, const double *px,
                     const double *py, const int32_t *cell, const int32_t *start, const double *cell_x,
                     const double *cell_y, const int32_t *cell_city, OrOptCand *cand, uint32_t *count,
                     hipStream_t stream)
{
    void *args[] = {&L, &g, &ring, &ord, &pos, &px, &py, &cell, &start, &cell_x, &cell_y, &cell_city, &cand, &count};
    return hipLaunchKernel(reinterpret_cast<const void *>(&or_opt_search_kernel<SEG>),
                           dim3(oo_grid((int64_t)L - 2)), dim3(kOoThreads), args, 0, stream);
}

}  // namespace

hipError_t launch_or_opt_search(int L, int g, int ring, int max_seg, const int32_t *ord, const int32_t *pos,
                                const double *px, const double *py, const int32_t *cell, const int32_t *start,
                                const double *cell_x, const double *cell_y, const int32_t *cell_city,
                                OrOptCand *cand, uint32_t *count, hipStream_t stream)
{
    if (L < 4 || g < 1 || g > kTwoOptMaxGrid || ring < 1 || ring > kTwoOptMaxRing) return hipErrorInvalidValue;
    switch (max_seg) {
    case 1:
        return oo_search<1>(L, g, ring, ord, pos, px, py, cell, start, cell_x, cell_y, cell_city, cand, count, stream);
    case 2:
        return oo_search<2>(L, g, ring, ord, pos, px, py, cell, start, cell_x, cell_y, cell_city, cand, count, stream);
    case 3:
        return oo_search<3>(L, g, ring, ord, pos, px, py, cell, start, cell_x, cell_y, cell_city, cand, count, stream);
    default:
        return hipErrorInvalidValue;
    }
}

hipError_t launch_or_opt_apply(int moves, const int32_t *acc_lo, const int32_t *acc_hi, const int32_t *acc_how,
                               const int32_t *prefix, int total, int L, int32_t *ord, int32_t *pos, double *px,
                               double *py, int32_t *s_ord, double *s_x, double *s_y, hipStream_t stream)
{
    if (moves <= 0 || total <= 0) return hipSuccess;
    if (total >= L) return hipErrorInvalidValue;  // the scratch arrays hold L
    const dim3 grid(oo_grid(total)), block(kOoThreads);
    void *a1[] = {&moves, &acc_lo, &acc_hi, &acc_how, &prefix, &total, &ord, &px, &py, &s_ord, &s_x, &s_y};
    const hipError_t e =
        hipLaunchKernel(reinterpret_cast<const void *>(&or_opt_stage_kernel), grid, block, a1, 0, stream);
    if (e != hipSuccess) return e;
    void *a2[] = {&moves, &acc_lo, &acc_hi, &acc_how, &prefix, &total, &L, &s_ord, &s_x, &s_y, &ord, &pos, &px, &py};
    return hipLaunchKernel(reinterpret_cast<const void *>(&or_opt_commit_kernel), grid, block, a2, 0, stream);
}

}  // namespace tspgpu
