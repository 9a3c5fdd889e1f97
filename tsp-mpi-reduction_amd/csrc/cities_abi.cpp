// C-ABI of libtspgpu (include/tspgpu.h): distances on the device (DESIGN.md
// §4e) — cities in HBM -> the reference's matrices, bit for bit — and the
// forms that solve from cities.  Build kernel (x*x everywhere, the squares
// where glibc's pow may differ listed) -> one synchronisation, the host's pow
// on the listed operands -> patch + finish kernels (cities.hip, dist_exact.h).
#include "tspgpu.h"
#include "tuning.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <mutex>
#include <vector>

#include "abi_internal.h"
#include "cities.h"

using namespace tspgpu;

int tspgpu::cities_args(const tspgpu_ctx *c, const void *cities, int n, const int32_t *ns, bool ragged, int nblocks,
                        int min_n, int *max_n, int64_t *ncities)
{
    if (!c || nblocks < 0) return -EINVAL;
    if (!ragged && (n < min_n || n > TSPGPU_MAX_CITIES)) return -EINVAL;
    if (nblocks > 0 && (!cities || (ragged && !ns))) return -EINVAL;
    if (!ragged && min_n >= 2)
        if (const int rc = check_n(n, c->strict)) return rc;  // (c is read from here on)
    if (nblocks == 0) return 1;
    *max_n = ragged ? 0 : n;
    *ncities = ragged ? 0 : (int64_t)nblocks * n;
    for (int b = 0; ragged && b < nblocks; ++b) {
        if (ns[b] < min_n || ns[b] > TSPGPU_MAX_CITIES) return -EINVAL;
        *max_n = std::max(*max_n, (int)ns[b]);
        *ncities += ns[b];
    }
    return 0;
}

namespace {

// The descriptor table of packed ragged blocks (block_desc.h) onto the device
// on `stream`, through the context's pinned upload (bd_desc).  Blocks of more
// than skip_above cities get n = 0: the build skips them, the offsets still
// count them.  -> *out (the context's table).
int upload_block_desc(tspgpu_ctx *c, const int32_t *ns, int skip_above, int nblocks, hipStream_t stream,
                      const BlockDesc **out)
{
    const size_t bytes = (size_t)nblocks * sizeof(BlockDesc);
    void *h = nullptr;
    int rc = c->bd_desc.begin(bytes, &h);
    if (rc) return rc;
    BlockDesc *hd = static_cast<BlockDesc *>(h);
    int64_t city = 0, dist = 0, path = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int k = ns[b], L = tspgpu_tour_length(k);
        hd[b] = BlockDesc{city, dist, path, k > skip_above ? 0 : k, L};
        city += k;
        dist += (int64_t)k * k;
        path += L;
    }
    if ((rc = c->bd_desc.enqueue(bytes, stream))) return rc;
    *out = static_cast<const BlockDesc *>(c->bd_desc.dev.p);
    return 0;
}

}  // namespace

// (abi_internal.h: the window refinement builds its windows' matrices with it)
int tspgpu::cities_build_locked(tspgpu_ctx *c, const tspgpu_city *d_cities, int n, int nblocks, double *d_dist,
                                hipStream_t stream, const int32_t *ns, int skip_above)
{
    using clk = std::chrono::steady_clock;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    unsigned long long squares = (unsigned long long)nblocks * n * (n - 1);
    if (ns) {
        squares = 0;
        for (int b = 0; b < nblocks; ++b)
            if (ns[b] <= skip_above) squares += (unsigned long long)ns[b] * (ns[b] - 1);
    }
    // list capacity: a quarter of the squares (the rule flags a tenth of the
    // generator's), or the test knob; an overflowing build is run again
    unsigned long long cap = squares / 4;
    double kv = 0.0;
    if (tspgpu::tuned("DIST_FIX_CAP", &kv) && kv >= 1.0) cap = (unsigned long long)kv;
    if (cap > squares) cap = squares;
    if (cap < 1) cap = 1;
    int rc = 0;
    hipError_t e = hipSuccess;
    if ((rc = dev_reserve(c->d_ct_count, sizeof(unsigned long long)))) return rc;
    if ((rc = pinned_reserve(c->h_ct_count, sizeof(unsigned long long)))) return rc;
    // the list and the pinned buffers are the context's: under the workspace
    // ordering rule
    if ((rc = workspace_wait(c, stream))) return rc;
    const BlockDesc *desc = nullptr;
    if (ns && (rc = upload_block_desc(c, ns, skip_above, nblocks, stream, &desc))) return rc;
    const auto t0 = clk::now();
    unsigned long long count = 0;
    int passes = 0;
    for (;;) {
        const size_t lb = (size_t)cap * sizeof(double);
        if ((rc = dev_reserve(c->d_ct_slot, (size_t)cap * sizeof(int64_t)))) return rc;
        if ((rc = dev_reserve(c->d_ct_dx, lb))) return rc;
        if (c->h_ct_fix.cap < lb) {
            // (growing: an earlier build's copy of its results, on another
            // stream, may still be reading the old buffer)
            if (c->h_ct_fix && (e = hipDeviceSynchronize()) != hipSuccess) return hip_err(e);
            if ((rc = pinned_reserve(c->h_ct_fix, lb))) return rc;
        }
        e = hipMemsetAsync(c->d_ct_count, 0, sizeof(unsigned long long), stream);
        if (e == hipSuccess)
            e = desc ? launch_cities_build_ragged(d_cities, desc, nblocks, d_dist, c->d_ct_slot, c->d_ct_dx, cap,
                                                  c->d_ct_count, stream)
                     : launch_cities_build(d_cities, n, nblocks, d_dist, c->d_ct_slot, c->d_ct_dx, cap, c->d_ct_count,
                                           stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->h_ct_count, c->d_ct_count, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->h_ct_fix, c->d_ct_dx, lb, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_err(e);
        ++passes;
        count = *c->h_ct_count.p;
        if (count <= cap) break;
        if (passes >= 2 || count > squares) return -EIO;  // (the build is deterministic: the second pass fits)
        cap = count;
    }
    const auto t1 = clk::now();
    // the host's pow on the flagged operands, in place, on up to 16 threads
    // from 2^16 operands
    double *v = c->h_ct_fix;
    parallel_ranges((size_t)count, 16, (size_t)1 << 16, [v](size_t a, size_t b) {
        for (size_t t = a; t < b; ++t) v[t] = pow_fn(v[t], 2);
    });
    const auto t2 = clk::now();
    if (count)
        e = hipMemcpyAsync(c->d_ct_dx, v, (size_t)count * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = launch_cities_patch(d_dist, c->d_ct_slot, c->d_ct_dx, count, stream);
    if (e == hipSuccess)
        e = desc ? launch_cities_finish_ragged(desc, nblocks, d_dist, stream)
                 : launch_cities_finish(n, nblocks, d_dist, stream);
    if (e != hipSuccess) return hip_err(e);
    if ((rc = workspace_done(c, stream))) return rc;
    c->ct_squares = squares;
    c->ct_flagged = count;
    c->ct_passes = passes;
    c->ct_build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->ct_pow_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return 0;
}

namespace {

// Build the matrices into the context's buffer, then the ragged path (c->mu
// held): n cities for every block, or, with ns, packed blocks of ns[b] cities
// at the packed offsets.  On a strict context a block of 17..20 cities is
// refused by the plan (status -EINVAL) and its matrix is not built.
int cities_solve_locked(tspgpu_ctx *c, const tspgpu_city *d_cities, int n, const int32_t *ns, int nblocks,
                        double *d_cost, int32_t *d_tour, int tour_stride, int32_t *d_status, hipStream_t stream)
{
    std::vector<int32_t> same(ns ? 0 : (size_t)nblocks, n);
    const int32_t *sizes = ns ? ns : same.data();
    std::vector<int64_t> offset((size_t)nblocks);
    int64_t elems = 0;
    for (int b = 0; b < nblocks; ++b) {
        offset[b] = elems;
        elems += (int64_t)sizes[b] * sizes[b];
    }
    RaggedPlan plan;
    int rc = ragged_plan(sizes, offset.data(), nblocks, c->strict, 8, &plan);
    if (rc) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    if ((rc = dev_reserve(c->d_ct_dist, (size_t)elems * sizeof(double)))) return rc;
    const int skip_above = c->strict ? TSPGPU_REFERENCE_MAX_CITIES : TSPGPU_MAX_CITIES;
    if ((rc = cities_build_locked(c, d_cities, n, nblocks, c->d_ct_dist, stream, ns, skip_above))) return rc;
    return ragged_locked(c, c->d_ct_dist, 8, plan, 0, d_cost, d_tour, tour_stride, d_status, stream);
}

// The host form of either: the cities up, cities_solve_locked, cost, tour and
// status down into the caller's arrays (c->mu held, the device set).
int cities_round_trip(tspgpu_ctx *c, const tspgpu_city *cities, int64_t ncities, int n, const int32_t *ns, int nblocks,
                      double *cost_out, int32_t *tour_out, int tour_stride, int32_t *status_out)
{
    auto run = [&] {
        return cities_solve_locked(c, reinterpret_cast<const tspgpu_city *>(c->d_ct_cities.p), n, ns, nblocks,
                                   reinterpret_cast<double *>(c->d_cost.p), reinterpret_cast<int32_t *>(c->d_tour.p),
                                   tour_stride, reinterpret_cast<int32_t *>(c->d_rg_ostatus.p), c->stream);
    };
    return host_round_trip(c, {&c->d_ct_cities, const_cast<tspgpu_city *>(cities), (size_t)ncities * sizeof(tspgpu_city)},
                           run,
                           {{&c->d_cost, cost_out, (size_t)nblocks * sizeof(double)},
                            {&c->d_tour, tour_out, (size_t)nblocks * tour_stride * sizeof(int32_t)},
                            {&c->d_rg_ostatus, status_out, (size_t)nblocks * sizeof(int32_t)}});
}

}  // namespace

extern "C" {

int tspgpu_distance_matrix_ragged_device(tspgpu_ctx *c, const tspgpu_city *d_cities, const int32_t *n, int nblocks,
                                         double *d_dist, void *hip_stream)
{
    int max_n = 0;
    int64_t ncities = 0;
    const int rc = cities_args(c, d_cities, 0, n, true, nblocks, 1, &max_n, &ncities);
    if (rc) return rc < 0 ? rc : 0;
    if (!d_dist) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return cities_build_locked(c, d_cities, 0, nblocks, d_dist, (hipStream_t)hip_stream, n);
}

int tspgpu_solve_cities_ragged_device(tspgpu_ctx *c, const tspgpu_city *d_cities, const int32_t *n, int nblocks,
                                      double *d_cost, int32_t *d_tour, int tour_stride, int32_t *d_status,
                                      void *hip_stream)
{
    int max_n = 0;
    int64_t ncities = 0;
    const int rc = cities_args(c, d_cities, 0, n, true, nblocks, 2, &max_n, &ncities);
    if (rc) return rc < 0 ? rc : 0;
    if (!d_cost || !d_tour || !d_status || tour_stride < max_n + 1) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return cities_solve_locked(c, d_cities, 0, n, nblocks, d_cost, d_tour, tour_stride, d_status,
                               (hipStream_t)hip_stream);
}

int tspgpu_solve_cities_ragged(tspgpu_ctx *c, const tspgpu_city *cities, const int32_t *n, int nblocks,
                               double *cost_out, int32_t *tour_out, int tour_stride, int32_t *status_out)
{
    int max_n = 0;
    int64_t ncities = 0;
    const int rc = cities_args(c, cities, 0, n, true, nblocks, 2, &max_n, &ncities);
    if (rc) return rc < 0 ? rc : 0;
    if (!cost_out || !tour_out || !status_out || tour_stride < max_n + 1) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    // (0 however many blocks are bad: status_out says which)
    return cities_round_trip(c, cities, ncities, 0, n, nblocks, cost_out, tour_out, tour_stride, status_out);
}

int tspgpu_distance_matrix_device(tspgpu_ctx *c, const tspgpu_city *d_cities, int n, int nblocks, double *d_dist,
                                  void *hip_stream)
{
    int max_n = 0;
    int64_t ncities = 0;
    const int rc = cities_args(c, d_cities, n, nullptr, false, nblocks, 1, &max_n, &ncities);
    if (rc) return rc < 0 ? rc : 0;
    if (!d_dist) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return cities_build_locked(c, d_cities, n, nblocks, d_dist, (hipStream_t)hip_stream);
}

int tspgpu_solve_cities_device(tspgpu_ctx *c, const tspgpu_city *d_cities, int n, int nblocks, double *d_cost,
                               int32_t *d_tour, int32_t *d_status, void *hip_stream)
{
    int max_n = 0;
    int64_t ncities = 0;
    const int rc = cities_args(c, d_cities, n, nullptr, false, nblocks, 2, &max_n, &ncities);
    if (rc) return rc < 0 ? rc : 0;
    if (!d_cost || !d_tour || !d_status) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return cities_solve_locked(c, d_cities, n, nullptr, nblocks, d_cost, d_tour, n + 1, d_status,
                               (hipStream_t)hip_stream);
}

int tspgpu_solve_cities_upload(tspgpu_ctx *c, const tspgpu_city *cities, int n, int nblocks, double *cost_out,
                               int32_t *tour_out)
{
    int max_n = 0;
    int64_t ncities = 0;
    int rc = cities_args(c, cities, n, nullptr, false, nblocks, 2, &max_n, &ncities);
    if (rc) return rc < 0 ? rc : 0;
    if (!cost_out || !tour_out) return -EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    std::vector<int32_t> status((size_t)nblocks);
    rc = cities_round_trip(c, cities, ncities, n, nullptr, nblocks, cost_out, tour_out, n + 1, status.data());
    if (rc) return rc;
    for (int b = 0; b < nblocks; ++b)
        if (status[b]) return status[b];  // the first bad block's code, as tspgpu_solve_cities
    return 0;
}

int tspgpu_cities_last_fixups(const tspgpu_ctx *c, uint64_t *squares, uint64_t *flagged, int *build_passes)
{
    if (!c) return -EINVAL;
    if (squares) *squares = c->ct_squares;
    if (flagged) *flagged = c->ct_flagged;
    if (build_passes) *build_passes = c->ct_passes;
    return 0;
}

int tspgpu_cities_last_phase_ms(const tspgpu_ctx *c, double *build_ms, double *pow_ms)
{
    if (!c) return -EINVAL;
    if (build_ms) *build_ms = c->ct_build_ms;
    if (pow_ms) *pow_ms = c->ct_pow_ms;
    return 0;
}

}  // extern "C"
