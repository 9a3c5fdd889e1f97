// C-ABI of libtspgpu (include/tspgpu.h): validation and the launch of the K1
// Held-Karp kernels (heldkarp.hip) — tables, slots, the dispatch by size.
//
// Replaces the reference's `BlockSolution tsp(vector<City>)` (tsp.cpp:405-509)
// for a whole batch of blocks in one call.  The distance matrix stays on the
// host (computeDistanceMatrix, assignment2.h:184-200) by default because glibc
// pow(x,2) differs from x*x in ~0.08% of inputs; the device forms
// (tspgpu_distance_matrix_device, cities_abi.cpp) send the host only the
// squares where it can differ.
#include "tspgpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "abi_internal.h"
#include "heldkarp.h"
#include "k1_cfg.h"

namespace tspgpu {

double (*volatile pow_fn)(double, double) = ::pow;
double (*volatile sqrt_fn)(double) = ::sqrt;

static int binom_host(int a, int b)
{
    if (b < 0 || b > a) return 0;
    long long r = 1;
    for (int i = 1; i <= b; ++i) r = r * (a - b + i) / i;
    return (int)r;
}

size_t table_doubles(int N) { return (size_t)N << (N - 1); }

void host_layer_info(int N, LayerInfo *info)
{
    std::memset(info, 0, sizeof(*info));
    for (int a = 0; a < kBinomRows; ++a)
        for (int b = 0; b < kBinomCols; ++b) info->binom[a * kBinomCols + b] = binom_host(a, b);
    // colex rank = sum over members e_i (ascending) of C(e_i, i+1), split in
    // three 7-bit digit groups whose contribution depends on the member count below
    for (int lo = 0; lo < 128; ++lo) {
        int r = 0, i = 0;
        for (int b = 0; b < 7; ++b)
            if (lo >> b & 1) r += binom_host(b, ++i);
        info->rlut[lo] = r;
    }
    for (int mid = 0; mid < 128; ++mid)
        for (int c = 0; c < 8; ++c) {
            int r = 0, i = c;
            for (int b = 0; b < 7; ++b)
                if (mid >> b & 1) r += binom_host(b + 7, ++i);
            info->rlut[kRankR1 + mid * 8 + c] = r;
        }
    for (int hi = 0; hi < 64; ++hi)
        for (int c = 0; c < 15; ++c) {
            int r = 0, i = c;
            for (int b = 0; b < 6; ++b)
                if (hi >> b & 1) r += binom_host(b + 14, ++i);
            info->rlut[kRankR1 + kRankR2 + hi * 15 + c] = r;
        }
    int off = 0, moff = 0;
    for (int t = 0; t <= N + 1 && t < 24; ++t) {
        info->count[t] = binom_host(N, t);
        info->moff[t] = moff;
        moff += info->count[t];
        if (t >= 1) {
            info->off[t] = off;
            off += info->count[t] * t;
        }
    }
}

}  // namespace tspgpu

using namespace tspgpu;

namespace {

// a one-time table upload on the context's stream (xfer.h: small tables skip
// the runtime's copy path and its first-use cost)
hipError_t upload_sync(tspgpu_ctx *c, void *d, const void *h, size_t bytes)
{
    hipError_t e = xcopy_async(d, h, bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

int ensure_tables(tspgpu_ctx *c, int N)
{
    if (c->d_info[N]) return 0;
    LayerInfo info;
    host_layer_info(N, &info);
    // every N-bit mask by (popcount, value): each popcount class in ascending
    // order by Gosper's next-combination step (O(2^N), not (N+1) 2^N scans)
    std::vector<uint32_t> masks;
    masks.reserve((size_t)1 << N);
    masks.push_back(0u);
    for (int t = 1; t <= N; ++t)
        for (uint32_t m = (1u << t) - 1u; m < (1u << N);) {
            masks.push_back(m);
            const uint32_t c = m & (0u - m), r = m + c;
            m = (((r ^ m) >> 2) / c) | r;
        }
    DevBuf<LayerInfo> d_info;
    DevBuf<uint32_t> d_masks;
    hipError_t e = dev_alloc(d_info, 1);
    if (e == hipSuccess) e = dev_alloc(d_masks, masks.size());
    if (e == hipSuccess) e = upload_sync(c, d_info, &info, sizeof(info));
    if (e == hipSuccess) e = upload_sync(c, d_masks, masks.data(), masks.size() * sizeof(uint32_t));
    if (e != hipSuccess) return hip_err(e);
    c->d_info[N] = std::move(d_info);
    c->d_masks[N] = std::move(d_masks);
    return 0;
}

int ensure_tiled_info(tspgpu_ctx *c, int L)
{
    if (c->d_tinfo[L]) return 0;
    auto info = std::make_unique<TiledInfo>();
    std::memset(info.get(), 0, sizeof(TiledInfo));
    int k = 0;
    for (int j = 0; j <= L; ++j) {
        info->moff[j] = k;
        info->cnt[j] = binom_host(L, j);
        int r = 0;
        for (uint32_t m = 0; m < (1u << L); ++m)
            if (__builtin_popcount(m) == j) {  // numeric order of equal-popcount masks = colex order
                info->mask[k++] = (uint16_t)m;
                info->rankb8[m] = (uint16_t)(r * 8);
                info->rankb4[m] = (uint16_t)(r * 4);
                info->rank[m] = (uint16_t)r++;
            }
    }
    info->moff[L + 1] = k;
    DevBuf<void> d;
    if (int rc = dev_reserve(d, sizeof(TiledInfo))) return rc;
    if (hipError_t e = upload_sync(c, d, info.get(), sizeof(TiledInfo)); e != hipSuccess) return hip_err(e);
    c->d_tinfo[L] = std::move(d);
    return 0;
}

// Variant 6 keeps one global slot per block of a launch (sized by the
// configuration in use: 1.65 MB at n = 16 with ten low cities, 1.49 MB with
// eleven) until its backtracking kernel has run, so a launch takes blocks in
// chunks: up to 65536 (108 GB of the 288 GB at n = 16 — a persistent grid of
// 1536 workgroups then idles a third of the chip for 0.67 of 42.7 rounds
// instead of 0.67 of 10.7 at 16384), at most 3/4 of the device memory free
// at that moment (other contexts or ranks on the same GPU keep theirs),
// halved while the allocation fails, down to 64 blocks.  A slot area far
// larger than a later launch needs (> 4x and > 8 GB) is given back first.
// (The knob K1_CHUNK lowers the 65536 so that tests can run several chunks
// from a small batch.)
int ensure_slots(tspgpu_ctx *c, int nblocks, size_t slot, int *chunk)
{
    int ch = std::min(nblocks, c->k1_chunk);
    const size_t need = (size_t)ch * slot;
    if (c->d_tslots.cap > 4 * need && c->d_tslots.cap > ((size_t)8 << 30)) c->d_tslots.reset();
    if (c->d_tslots.cap < need) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t usable = (free_b + c->d_tslots.cap) / 4 * 3;  // (the current area is freed first)
            while (ch > 64 && (size_t)ch * slot > usable) ch /= 2;
        }
    }
    for (;;) {
        const int rc = dev_reserve(c->d_tslots, (size_t)ch * slot);
        if (rc == 0 || rc != -ENOMEM || ch <= 64) {
            *chunk = ch;
            return rc;
        }
        (void)hipGetLastError();  // (clear the failed allocation's error)
        ch /= 2;
    }
}

// Split timing (tspgpu_k1_split_timing): three events per chunk, kept until
// tspgpu_k1_last_split_ms reads them; the first is recorded here.  *ev0 = the
// chunk's first event index (unused when split timing is off).
int split_begin(tspgpu_ctx *c, hipStream_t stream, size_t *ev0)
{
    *ev0 = 0;
    if (!c->split_timing) return 0;
    constexpr size_t kMaxEvents = 3 * 4096;
    if (c->split_used + 3 > kMaxEvents) {  // more chunks than the pool: stop recording
        c->split_overflow = true;
        c->split_timing = 0;
        return 0;
    }
    while (c->ev_split.size() < c->split_used + 3) {
        Event ev;
        if (hipEventCreate(&ev.p) != hipSuccess) return -EIO;
        c->ev_split.push_back(std::move(ev));
    }
    *ev0 = c->split_used;
    c->split_used += 3;
    return hipEventRecord(c->ev_split[*ev0], stream) == hipSuccess ? 0 : -EIO;
}

// Variant 6 row table of L (sub_rows.h, built by sub_rows.cpp), uploaded once.
int ensure_sub_rows(tspgpu_ctx *c, int L)
{
    if (L < 0 || L >= 16) return -EINVAL;
    if (c->d_subrows[L]) return 0;
    std::vector<SubRow> rows;
    if (!build_sub_rows(L, rows)) return -EINVAL;
    int rc = ensure_tiled_info(c, L);
    if (rc) return rc;
    DevBuf<void> d;
    if ((rc = dev_reserve(d, rows.size() * sizeof(SubRow)))) return rc;
    if (hipError_t e = upload_sync(c, d, rows.data(), rows.size() * sizeof(SubRow)); e != hipSuccess) return hip_err(e);
    c->d_subrows[L] = std::move(d);
    return 0;
}

// K1 variant 6 (hk_sub.h) configuration for (N, value bytes): the one
// TSPGPU_TILED_CFG names, else the first row of the table; null if none.
const SubCfg *pick_sub(const tspgpu_ctx *c, int N, int vbytes)
{
    int cnt = 0;
    const SubCfg *t = sub_cfgs(&cnt);
    if (c->tiled_cfg >= 0) {
        for (int i = 0; i < cnt; ++i)
            if (t[i].id == c->tiled_cfg && t[i].N == N && t[i].vbytes == vbytes) return &t[i];
        return nullptr;
    }
    for (int i = 0; i < cnt; ++i)
        if (t[i].N == N && t[i].vbytes == vbytes) return &t[i];
    return nullptr;
}

int solve_sub(tspgpu_ctx *c, const SubCfg *cfg, const void *d_dist, int n, int nblocks, void *d_cost,
              int32_t *d_tour, hipStream_t stream)
{
    const int N = n - 1, L = cfg->L;
    int rc = ensure_sub_rows(c, L);
    if (rc) return rc;
    // (TSPGPU_WG_PER_CU: measurement builds with another occupancy, hk_sub.h)
    const int grid = std::min(nblocks, c->cu_count * (c->wg_per_cu > 0 ? c->wg_per_cu : cfg->wg));
    // the per-block slot (push area, parent words, recompute area:
    // hk_tiled.h), kept until the backtracking kernel has run
    const size_t slot = sub_slot_bytes(N, L, cfg->vbytes);
    int chunk = 0;
    if ((rc = ensure_slots(c, nblocks, slot, &chunk))) return rc;
    for (int b0 = 0; b0 < nblocks; b0 += chunk) {
        SubArgs a{};
        size_t ev0 = 0;
        if ((rc = split_begin(c, stream, &ev0))) return rc;
        a.ev_mid = c->split_timing ? c->ev_split[ev0 + 1].p : nullptr;
        a.dist = d_dist;
        a.n = n;
        a.blk0 = b0;
        a.blk1 = std::min(nblocks, b0 + chunk);
        a.slots = c->d_tslots;
        a.slot_bytes = (uint32_t)slot;
        a.rows = static_cast<const SubRow *>(c->d_subrows[L].p);
        a.info = static_cast<const TiledInfo *>(c->d_tinfo[L].p);
        a.cost = d_cost;
        a.tour = d_tour;
        a.grid = std::min(grid, a.blk1 - a.blk0);
        a.bt_grid = std::min((a.blk1 - a.blk0 + kTiledBtWaves - 1) / kTiledBtWaves, c->cu_count * TSPGPU_TILED_BTWG);
        a.stream = stream;
        hipError_t e = cfg->launch(a);
        if (e != hipSuccess) return hip_err(e);
        if (c->split_timing && hipEventRecord(c->ev_split[ev0 + 2], stream) != hipSuccess) return -EIO;
    }
    c->last_grid = grid;
    c->last_variant = 6;
    return 0;
}

int solve_device_unordered(tspgpu_ctx *c, const void *d_dist, int n, int nblocks, void *d_cost, int32_t *d_tour,
                           hipStream_t stream, int vbytes);

}  // namespace

int tspgpu::check_n(int n, int strict)
{
    if (n < 2) return -EINVAL;
    if (n > (strict ? TSPGPU_REFERENCE_MAX_CITIES : TSPGPU_MAX_CITIES)) return -EINVAL;
    return 0;
}

// one launch under the workspace ordering rule (abi_internal.h)
int tspgpu::solve_device_locked(tspgpu_ctx *c, const void *d_dist, int n, int nblocks, void *d_cost, int32_t *d_tour,
                                hipStream_t stream, int vbytes)
{
    int rc = 0;
    if (nblocks > 0) {
        if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
        if ((rc = workspace_wait(c, stream))) return rc;
    }
    rc = solve_device_unordered(c, d_dist, n, nblocks, d_cost, d_tour, stream, vbytes);
    if (rc || nblocks <= 0) return rc;
    return workspace_done(c, stream);
}

namespace {

int solve_device_unordered(tspgpu_ctx *c, const void *d_dist, int n, int nblocks, void *d_cost, int32_t *d_tour,
                           hipStream_t stream, int vbytes)
{
    int rc = check_n(n, c->strict);
    if (rc) return rc;
    if (nblocks < 0 || (nblocks > 0 && (!d_dist || !d_cost || !d_tour))) return -EINVAL;
    if (nblocks == 0) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    const int N = n - 1;
    LaunchArgs a{};
    a.dist = d_dist;
    a.n = n;
    a.nblocks = nblocks;
    a.cost = d_cost;
    a.tour = d_tour;
    a.stream = stream;
    a.vbytes = vbytes;
    int grid = nblocks;
    if (N >= 2) {
        rc = ensure_tables(c, N);
        if (rc) return rc;
        a.masks = c->d_masks[N];
        a.info = c->d_info[N];
        a.use_lds = N <= c->lds_table_max_n;
        // per-N defaults measured on MI355X (profiles/r01/*sweep*.log): small
        // tables want many blocks in flight; at n = 15, 16 one 1024-thread slot
        // per CU keeps the live layers of the 256 resident blocks in the
        // Infinity Cache (n = 15: 1.45x over two 512-thread slots)
        // (i32 tables are half the bytes: 512-thread pairs at n = 15, 16 and
        // 8 workgroups per CU up to n = 13; profiles/r01/i32_sweep*.log)
        int def_threads = N <= 11 ? 256 : (N <= 13 ? 512 : (N <= 15 ? 1024 : 256));
        int def_wg = N <= 11 ? 8 : (N <= 13 ? 2 : (N <= 15 ? 1 : 2));
        if (vbytes == 4) {
            def_threads = N <= 13 ? 256 : (N <= 15 ? 512 : 256);
            def_wg = N <= 12 ? 8 : (N <= 13 ? 4 : 2);
        }
        a.threads = c->threads > 0 ? c->threads : def_threads;
        // a full wave of blocks: the sub-cube kernel, variant 6 (hk_sub.h), at
        // 13-16 cities f64 and 16 cities i32, the compact layer pass (variant
        // 2) elsewhere (measurements per size: DESIGN.md §4.0, §4.0a)
        const bool tiled = vbytes == 8 ? (N >= 12 && N <= 15) : N == 15;
        a.variant = c->variant >= 0 ? c->variant : (tiled && nblocks >= c->cu_count ? 6 : 2);
        if (a.variant == 6) {
            if (const SubCfg *cfg = pick_sub(c, N, vbytes))
                return solve_sub(c, cfg, d_dist, n, nblocks, d_cost, d_tour, stream);
        }
        // no variant-6 configuration for this size (or K1=5, the retired
        // variant 5, kept as an alias of this fall-back): ping-pong + parents
        // pays at 16 cities f64 (the two live middle layers of all resident
        // blocks then stay in the Infinity Cache), not below
        if (a.variant >= 5) a.variant = vbytes == 8 && N == 15 ? 4 : 2;
        // variant 4 at 16 cities: one 512-thread workgroup per CU at 2 waves/SIMD
        // (256 VGPRs; heldkarp_impl.h TSPGPU_K1_WAVES_512V4) beats 1024 threads at 4
        if (c->threads <= 0 && a.variant == 4 && N == 15 && vbytes == 8) a.threads = 512;
        if (a.use_lds) {
            // as many resident workgroups as the LDS allows, then persistent
            const int per_cu = (int)(160 * 1024 / lds_bytes_for(N, true, threads_for(N, true, 0), vbytes));
            const int cap = c->cu_count * (per_cu > 0 ? per_cu : 1);
            grid = nblocks < cap ? nblocks : cap;
        } else {
            // extension sizes (N >= 16) run at 2 waves/SIMD: two workgroups per CU
            const int wg = c->wg_per_cu > 0 ? c->wg_per_cu : def_wg;
            const int per_cu = N >= 16 ? (wg < 2 ? wg : 2) : wg;
            int slots = c->slots_opt > 0 ? c->slots_opt : c->cu_count * per_cu;
            // keep the workspace under ~8 GiB for the largest extension sizes
            const size_t per = table_doubles(N) * (size_t)vbytes;
            const size_t budget = (size_t)8 << 30;
            if ((size_t)slots * per > budget) slots = (int)(budget / per);
            if (slots < 1) slots = 1;
            grid = nblocks < slots ? nblocks : slots;
            a.slot_doubles = table_doubles(N);
            rc = dev_reserve(c->d_slots, (size_t)grid * per);
            if (rc) return rc;
            a.slots = c->d_slots;
        }
    }
    c->last_grid = grid;
    c->last_variant = N >= 2 ? a.variant : 0;
    return hip_err(launch_heldkarp(a, grid));
}

thread_local std::unique_ptr<tspgpu_ctx, int (*)(tspgpu_ctx *)> t_default(nullptr, tspgpu_ctx_destroy);

template <typename V>
int solve_host_copy(tspgpu_ctx *c, const V *dist, int n, int nblocks, V *cost_out, int32_t *tour_out)
{
    if (nblocks > 0 && (!cost_out || !tour_out)) return -EINVAL;
    if (nblocks == 0) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    const size_t db = (size_t)nblocks * n * n * sizeof(V);
    const size_t cb = (size_t)nblocks * sizeof(V);
    const size_t tb = (size_t)nblocks * (n + 1) * sizeof(int32_t);
    auto run = [&] {
        int32_t *d_tour = reinterpret_cast<int32_t *>(c->d_tour.p);
        const hipError_t e = xset_async(d_tour, 0xff, tb, c->stream);
        if (e != hipSuccess) return hip_err(e);
        return solve_device_locked(c, c->d_dist, n, nblocks, c->d_cost, d_tour, c->stream, (int)sizeof(V));
    };
    const int rc = host_round_trip(c, {&c->d_dist, const_cast<V *>(dist), db}, run,
                                   {{&c->d_cost, cost_out, cb}, {&c->d_tour, tour_out, tb}});
    if (rc) return rc;
    for (int b = 0; b < nblocks; ++b)
        if (cost_out[b] < V(0)) return -EIO;  // backtracking found no predecessor
    return 0;
}

}  // namespace

extern "C" {

int tspgpu_distance_matrix(const tspgpu_city *cities, int n, int nblocks, double *dist)
{
    // assignment2.h:196: sqrt(pow(dx, 2) + pow(dy, 2)), glibc pow really called
    // (pow_fn, above)
    if (n < 1 || nblocks < 0 || (nblocks > 0 && (!cities || !dist))) return -EINVAL;
    auto run = [&](size_t b0, size_t b1) {
        for (size_t b = b0; b < b1; ++b) {
            const tspgpu_city *c = cities + b * n;
            double *d = dist + b * n * n;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    const double dx = pow_fn(c[i].x - c[j].x, 2);
                    const double dy = pow_fn(c[i].y - c[j].y, 2);
                    d[i * n + j] = sqrt_fn(dx + dy);
                }
        }
    };
    // large batches (a whole rank's blocks, 2^18 matrix entries and more) on
    // up to 16 host threads
    const size_t per = (size_t)n * n;
    parallel_ranges((size_t)nblocks, 16, (((size_t)1 << 18) + per - 1) / per, run);
    return 0;
}

int tspgpu_validate(const double *dist, int n, int nblocks, int strict)
{
    int rc = check_n(n, strict);
    if (rc) return rc;
    if (nblocks < 0 || (nblocks > 0 && !dist)) return -EINVAL;
    for (int b = 0; b < nblocks; ++b) {
        const double *d = dist + (size_t)b * n * n;
        double mx = 0.0;
        for (int i = 0; i < n * n; ++i) {
            const double v = d[i];
            // (-0.0 passes v >= 0.0: the kernels' v_min_f64 orders it below +0.0
            // where the reference's strict < keeps the first, so the sign of a
            // zero cost could differ from the reference's — refused)
            if (!(v >= 0.0) || std::signbit(v) || !std::isfinite(v)) return -EINVAL;
            if (v > mx) mx = v;
        }
        // Every partial tour has at most n edges: below INT_MAX the reference's
        // sentinel (tsp.cpp:411,453) never wins a comparison.
        if ((double)n * mx >= (double)INT_MAX) return -ERANGE;
    }
    return 0;
}

int tspgpu_solve_blocks_device(tspgpu_ctx *c, const double *d_dist, int n, int nblocks, double *d_cost,
                               int32_t *d_tour, void *hip_stream)
{
    if (!c) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return solve_device_locked(c, d_dist, n, nblocks, d_cost, d_tour, (hipStream_t)hip_stream, 8);
}

int tspgpu_solve_blocks_i32_device(tspgpu_ctx *c, const int32_t *d_dist, int n, int nblocks, int32_t *d_cost,
                                   int32_t *d_tour, void *hip_stream)
{
    if (!c) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return solve_device_locked(c, d_dist, n, nblocks, d_cost, d_tour, (hipStream_t)hip_stream, 4);
}

int tspgpu_solve_blocks(tspgpu_ctx *c, const double *dist, int n, int nblocks, double *cost_out,
                        int32_t *tour_out)
{
    if (!c) return -EINVAL;
    int rc = tspgpu_validate(dist, n, nblocks, c->strict);
    if (rc) return rc;
    return solve_host_copy(c, dist, n, nblocks, cost_out, tour_out);
}

int tspgpu_solve_blocks_i32(tspgpu_ctx *c, const int32_t *dist, int n, int nblocks, int32_t *cost_out,
                            int32_t *tour_out)
{
    if (!c) return -EINVAL;
    int rc = tspgpu_validate_i32(dist, n, nblocks, c->strict);
    if (rc) return rc;
    return solve_host_copy(c, dist, n, nblocks, cost_out, tour_out);
}

int tspgpu_validate_i32(const int32_t *dist, int n, int nblocks, int strict)
{
    int rc = check_n(n, strict);
    if (rc) return rc;
    if (nblocks < 0 || (nblocks > 0 && !dist)) return -EINVAL;
    for (int b = 0; b < nblocks; ++b) {
        const int32_t *d = dist + (size_t)b * n * n;
        int64_t mx = 0;
        for (int i = 0; i < n * n; ++i) {
            if (d[i] < 0) return -EINVAL;
            if (d[i] > mx) mx = d[i];
        }
        // n edges per tour stay below INT_MAX: no i32 overflow, and the same
        // sentinel argument as tspgpu_validate
        if ((int64_t)n * mx >= (int64_t)INT_MAX) return -ERANGE;
    }
    return 0;
}

int tspgpu_solve_cities(tspgpu_ctx *c, const tspgpu_city *cities, int n, int nblocks, double *cost_out,
                        int32_t *tour_out)
{
    if (n < 2 || nblocks < 0) return -EINVAL;
    std::vector<double> dist((size_t)nblocks * n * n);
    int rc = tspgpu_distance_matrix(cities, n, nblocks, dist.data());
    if (rc) return rc;
    return tspgpu_solve_blocks(c, dist.data(), n, nblocks, cost_out, tour_out);
}

int tspgpu_solve(const double *dist, int n, int nblocks, double *cost_out, int32_t *tour_out,
                 const tspgpu_opts *opts)
{
    if (!t_default) {
        tspgpu_ctx *c = nullptr;
        int rc = tspgpu_ctx_create(opts, &c);
        if (rc) return rc;
        t_default.reset(c);
    }
    t_default->strict = opts ? opts->strict : 0;
    return tspgpu_solve_blocks(t_default.get(), dist, n, nblocks, cost_out, tour_out);
}

int tspgpu_last_grid(const tspgpu_ctx *c) { return c ? c->last_grid : 0; }

int tspgpu_last_variant(const tspgpu_ctx *c) { return c ? c->last_variant : -1; }

int tspgpu_k1_split_timing(tspgpu_ctx *c, int enable)
{
    if (!c) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    c->split_timing = enable ? 1 : 0;
    c->split_used = 0;
    c->split_overflow = false;
    return 0;
}

int tspgpu_k1_last_split_ms(tspgpu_ctx *c, float *forward_ms, float *backtrack_ms)
{
    if (!c || !forward_ms || !backtrack_ms) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (c->split_overflow) return -ENOSPC;
    if (!c->split_used) return -ENOENT;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    hipError_t e = hipEventSynchronize(c->ev_split[c->split_used - 1]);
    double fw = 0.0, bt = 0.0;
    for (size_t i = 0; e == hipSuccess && i < c->split_used; i += 3) {
        float f = 0.f, b = 0.f;
        e = hipEventElapsedTime(&f, c->ev_split[i], c->ev_split[i + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&b, c->ev_split[i + 1], c->ev_split[i + 2]);
        fw += f;
        bt += b;
    }
    c->split_used = 0;
    *forward_ms = (float)fw;
    *backtrack_ms = (float)bt;
    return hip_err(e);
}

}  // extern "C"
