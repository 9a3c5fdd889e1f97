// C-ABI of libtspgpu (include/tspgpu.h): fixed-end shortest paths and the
// window refinement of a tour on the device.  A path problem
// of w cities is K1 on the folded (w-1) x (w-1) matrix (refine.h): fold ->
// the ragged path with one size, so every block is validated on the device ->
// the closing 0 of K1's tour becomes w-1.  The refinement tiles the path with
// windows (refine_plan.h) and runs, per pass: gather the windows -> the exact
// device distance build -> fold + identity cost -> K1 -> apply.
#include "tspgpu.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstring>
#include <mutex>
#include <vector>

#include "abi_internal.h"
#include "refine.h"
#include "refine_plan.h"

using namespace tspgpu;

namespace {

int paths_vbytes(int dtype) { return dtype == TSPGPU_F64 ? 8 : (dtype == TSPGPU_I32 ? 4 : 0); }

// the call-level checks of the path forms; 1: nothing to do (nblocks == 0)
int paths_args(const tspgpu_ctx *c, const void *in, int w, int nblocks, const void *cost, const void *order,
               const void *status)
{
    if (!c || nblocks < 0) return -EINVAL;
    if (w < 4 || w > TSPGPU_MAX_CITIES) return -EINVAL;
    if (const int rc = check_n(w - 1, c->strict)) return rc;
    if (nblocks == 0) return 1;
    if (!in || !cost || !order || !status) return -EINVAL;
    return 0;
}

// nblocks path problems of w cities from their w x w matrices at d_dist, on
// `stream` (c->mu held): cost, order rows of w entries and status under the
// ragged contract applied to the folded matrices.  d_old (f64 only): every
// block's identity-order cost too.  after_fold: recorded behind the fold
// kernels.  Nothing is waited for.
int paths_locked(tspgpu_ctx *c, const void *d_dist, int vbytes, int w, int nblocks, void *d_cost, int32_t *d_order,
                 int32_t *d_status, hipStream_t stream, double *d_old = nullptr, hipEvent_t after_fold = nullptr)
{
    const int n = w - 1;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    std::vector<int32_t> sizes((size_t)nblocks, n);
    std::vector<int64_t> offset((size_t)nblocks);
    for (int b = 0; b < nblocks; ++b) offset[b] = (int64_t)b * n * n;
    RaggedPlan plan;
    int rc = ragged_plan(sizes.data(), offset.data(), nblocks, c->strict, vbytes, &plan);
    if (rc) return rc;
    if ((rc = dev_reserve(c->d_rf_fold, (size_t)nblocks * n * n * vbytes))) return rc;
    // the folded matrices are the context's: under the workspace ordering rule
    if ((rc = workspace_wait(c, stream))) return rc;
    hipError_t e = launch_paths_fold(vbytes, d_dist, w, nblocks, c->d_rf_fold, stream);
    if (e == hipSuccess && d_old) e = launch_paths_identity_cost(static_cast<const double *>(d_dist), w, nblocks, d_old, stream);
    if (e == hipSuccess && after_fold) e = hipEventRecord(after_fold, stream);
    if (e != hipSuccess) return hip_err(e);
    if ((rc = ragged_locked(c, c->d_rf_fold, vbytes, plan, 0, d_cost, d_order, w, d_status, stream))) return rc;
    return hip_err(launch_paths_close(d_order, d_status, w, nblocks, stream));
}

// the same from cities on the device, through the exact build into the
// context's matrices (synchronises the stream as that build does)
int paths_cities_locked(tspgpu_ctx *c, const tspgpu_city *d_cities, int w, int nblocks, double *d_cost,
                        int32_t *d_order, int32_t *d_status, hipStream_t stream)
{
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    int rc = dev_reserve(c->d_ct_dist, (size_t)nblocks * w * w * sizeof(double));
    if (rc) return rc;
    if ((rc = cities_build_locked(c, d_cities, w, nblocks, c->d_ct_dist, stream))) return rc;
    return paths_locked(c, c->d_ct_dist, 8, w, nblocks, d_cost, d_order, d_status, stream);
}

int refine_events(tspgpu_ctx *c)
{
    for (tspgpu::Event &ev : c->ev_rf)
        if (!ev) {
            const hipError_t e = hipEventCreate(&ev.p);
            if (e != hipSuccess) return hip_err(e);
        }
    return 0;
}

// One pass over d_path on `stream` (c->mu held, the device set, p.windows >
// 0): synchronous.  Adds to *st; -> *replaced, the windows this pass replaced.
int refine_pass_locked(tspgpu_ctx *c, tspgpu_city *d_path, const RefinePass &p, tspgpu_refine_stats *st,
                       int64_t *replaced, hipStream_t stream)
{
    const int W = (int)p.windows;
    int rc = 0;
    if ((rc = dev_reserve(c->d_rf_cities, (size_t)p.cities * sizeof(tspgpu_city)))) return rc;
    if ((rc = dev_reserve(c->d_rf_dist, (size_t)p.dist * sizeof(double)))) return rc;
    if ((rc = dev_reserve(c->d_rf_cost, (size_t)W * sizeof(double)))) return rc;
    if ((rc = dev_reserve(c->d_rf_old, (size_t)W * sizeof(double)))) return rc;
    if ((rc = dev_reserve(c->d_rf_gain, (size_t)W * sizeof(double)))) return rc;
    if ((rc = dev_reserve(c->d_rf_tour, (size_t)p.cities * sizeof(int32_t)))) return rc;
    if ((rc = dev_reserve(c->d_rf_status, (size_t)W * sizeof(int32_t)))) return rc;
    if ((rc = dev_reserve(c->d_rf_flag, (size_t)W * sizeof(int32_t)))) return rc;
    if ((rc = pinned_reserve(c->h_rf_gain, (size_t)W * sizeof(double)))) return rc;
    if ((rc = pinned_reserve(c->h_rf_flag, (size_t)W * sizeof(int32_t)))) return rc;
    if ((rc = pinned_reserve(c->h_rf_status, (size_t)W * sizeof(int32_t)))) return rc;
    if ((rc = refine_events(c))) return rc;
    // the windows' buffers are the context's: under the workspace ordering rule
    if ((rc = workspace_wait(c, stream))) return rc;
    tspgpu_city *packed = reinterpret_cast<tspgpu_city *>(c->d_rf_cities.p);
    hipError_t e = hipEventRecord(c->ev_rf[0], stream);
    if (e == hipSuccess) e = launch_refine_gather(d_path, p.offset, p.stride, p.w, W, packed, stream);
    if (e != hipSuccess) return hip_err(e);
    if ((rc = workspace_done(c, stream))) return rc;
    if ((rc = cities_build_locked(c, packed, p.w, W, c->d_rf_dist, stream))) return rc;
    if ((e = hipEventRecord(c->ev_rf[1], stream)) != hipSuccess) return hip_err(e);
    if ((rc = paths_locked(c, c->d_rf_dist, 8, p.w, W, c->d_rf_cost, c->d_rf_tour, c->d_rf_status, stream,
                           c->d_rf_old, c->ev_rf[2])))
        return rc;
    e = hipEventRecord(c->ev_rf[3], stream);
    if (e == hipSuccess)
        e = launch_refine_apply(d_path, p.offset, p.stride, p.w, W, packed, c->d_rf_tour, c->d_rf_status,
                                c->d_rf_cost, c->d_rf_old, c->d_rf_gain, c->d_rf_flag, stream);
    if (e == hipSuccess) e = hipEventRecord(c->ev_rf[4], stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_rf_gain, c->d_rf_gain, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_rf_flag, c->d_rf_flag, (size_t)W * sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_rf_status, c->d_rf_status, (size_t)W * sizeof(int32_t), hipMemcpyDeviceToHost,
                           stream);
    if (e != hipSuccess) return hip_err(e);
    if ((rc = workspace_done(c, stream))) return rc;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return hip_err(e);
    // the host's left fold of the gains, in window order
    int64_t rep = 0;
    for (int k = 0; k < W; ++k) {
        if (c->h_rf_status.p[k] != 0) ++st->skipped;
        if (c->h_rf_flag.p[k]) {
            ++rep;
            st->gain = st->gain + c->h_rf_gain.p[k];
        }
    }
    st->windows += W;
    st->replaced += rep;
    *replaced = rep;
    float ms[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i)
        if ((e = hipEventElapsedTime(&ms[i], c->ev_rf[i], c->ev_rf[i + 1])) != hipSuccess) return hip_err(e);
    st->build_ms += ms[0];
    st->k1_ms += ms[2];
    st->fold_apply_ms += (double)ms[1] + ms[3];
    return 0;
}

// the call-level checks of both refinement forms
int refine_args(const tspgpu_ctx *c, const void *path, int L, int m, int max_passes)
{
    if (!c || !path || L < 2 || max_passes < 1) return -EINVAL;
    RefinePass p;
    return refine_pass(L, m, 0, c->strict, &p);
}

int refine_locked(tspgpu_ctx *c, tspgpu_city *d_path, int L, int m, int max_passes, tspgpu_refine_stats *st,
                  hipStream_t stream)
{
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    RefinePass p;
    int rc = refine_pass(L, m, 0, c->strict, &p);
    if (rc || p.windows == 0) return rc;  // too short for a window: nothing runs
    int64_t before = 0;
    for (int pass = 0;; ++pass) {
        if ((rc = refine_pass(L, m, pass, c->strict, &p))) return rc;
        int64_t replaced = 0;
        if (p.windows > 0 && (rc = refine_pass_locked(c, d_path, p, st, &replaced, stream))) return rc;
        st->passes = pass + 1;
        if (refine_stop(pass, max_passes, replaced, before)) break;
        before = replaced;
    }
    return 0;
}

}  // namespace

extern "C" {

int tspgpu_solve_paths_device(tspgpu_ctx *c, const void *d_dist, int dtype, int w, int nblocks, void *d_cost,
                              int32_t *d_order, int32_t *d_status, void *hip_stream)
{
    if (!paths_vbytes(dtype)) return -EINVAL;
    const int rc = paths_args(c, d_dist, w, nblocks, d_cost, d_order, d_status);
    if (rc) return rc < 0 ? rc : 0;
    std::lock_guard<std::mutex> g(c->mu);
    return paths_locked(c, d_dist, paths_vbytes(dtype), w, nblocks, d_cost, d_order, d_status,
                        (hipStream_t)hip_stream);
}

int tspgpu_solve_paths(tspgpu_ctx *c, const void *dist, int dtype, int w, int nblocks, void *cost_out,
                       int32_t *order_out, int32_t *status_out)
{
    const int vbytes = paths_vbytes(dtype);
    if (!vbytes) return -EINVAL;
    const int rc = paths_args(c, dist, w, nblocks, cost_out, order_out, status_out);
    if (rc) return rc < 0 ? rc : 0;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    auto run = [&] {
        return paths_locked(c, c->d_dist, vbytes, w, nblocks, c->d_cost, reinterpret_cast<int32_t *>(c->d_tour.p),
                            reinterpret_cast<int32_t *>(c->d_rg_ostatus.p), c->stream);
    };
    return host_round_trip(c, {&c->d_dist, const_cast<void *>(dist), (size_t)nblocks * w * w * vbytes}, run,
                           {{&c->d_cost, cost_out, (size_t)nblocks * vbytes},
                            {&c->d_tour, order_out, (size_t)nblocks * w * sizeof(int32_t)},
                            {&c->d_rg_ostatus, status_out, (size_t)nblocks * sizeof(int32_t)}});
}

int tspgpu_solve_paths_cities_device(tspgpu_ctx *c, const tspgpu_city *d_cities, int w, int nblocks, double *d_cost,
                                     int32_t *d_order, int32_t *d_status, void *hip_stream)
{
    const int rc = paths_args(c, d_cities, w, nblocks, d_cost, d_order, d_status);
    if (rc) return rc < 0 ? rc : 0;
    std::lock_guard<std::mutex> g(c->mu);
    return paths_cities_locked(c, d_cities, w, nblocks, d_cost, d_order, d_status, (hipStream_t)hip_stream);
}

int tspgpu_solve_paths_cities(tspgpu_ctx *c, const tspgpu_city *cities, int w, int nblocks, double *cost_out,
                              int32_t *order_out, int32_t *status_out)
{
    const int rc = paths_args(c, cities, w, nblocks, cost_out, order_out, status_out);
    if (rc) return rc < 0 ? rc : 0;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    auto run = [&] {
        return paths_cities_locked(c, reinterpret_cast<const tspgpu_city *>(c->d_ct_cities.p), w, nblocks,
                                   reinterpret_cast<double *>(c->d_cost.p), reinterpret_cast<int32_t *>(c->d_tour.p),
                                   reinterpret_cast<int32_t *>(c->d_rg_ostatus.p), c->stream);
    };
    return host_round_trip(c, {&c->d_ct_cities, const_cast<tspgpu_city *>(cities), (size_t)nblocks * w * sizeof(tspgpu_city)},
                           run,
                           {{&c->d_cost, cost_out, (size_t)nblocks * sizeof(double)},
                            {&c->d_tour, order_out, (size_t)nblocks * w * sizeof(int32_t)},
                            {&c->d_rg_ostatus, status_out, (size_t)nblocks * sizeof(int32_t)}});
}

int tspgpu_refine_path_device(tspgpu_ctx *c, tspgpu_city *d_path, int L, int m, int max_passes,
                              tspgpu_refine_stats *stats, void *hip_stream)
{
    const int rc = refine_args(c, d_path, L, m, max_passes);
    if (rc) return rc;
    tspgpu_refine_stats st;
    std::memset(&st, 0, sizeof st);
    int out = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        out = refine_locked(c, d_path, L, m, max_passes, &st, (hipStream_t)hip_stream);
    }
    if (stats) *stats = st;
    return out;
}

int tspgpu_refine_path(tspgpu_ctx *c, const tspgpu_city *path, int L, int m, int max_passes, tspgpu_city *path_out,
                       tspgpu_refine_stats *stats)
{
    const int rc = refine_args(c, path, L, m, max_passes);
    if (rc) return rc;
    if (!path_out) return -EINVAL;
    tspgpu_refine_stats st;
    std::memset(&st, 0, sizeof st);
    int out = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
        const size_t bytes = (size_t)L * sizeof(tspgpu_city);
        auto run = [&] {
            return refine_locked(c, reinterpret_cast<tspgpu_city *>(c->d_rf_path.p), L, m, max_passes, &st, c->stream);
        };
        out = host_round_trip(c, {&c->d_rf_path, const_cast<tspgpu_city *>(path), bytes}, run,
                              {{&c->d_rf_path, path_out, bytes}});
    }
    if (stats) *stats = st;
    return out;
}

int tspgpu_path_length(const tspgpu_city *path, int L, double *len)
{
    if (!path || !len || L < 1) return -EINVAL;
    // the reference's distance() (assignment2.h:141-144) on consecutive
    // cities, folded from the left; glibc pow really called (pow_fn)
    double s = 0.0;
    for (int i = 1; i < L; ++i) {
        const double dx = pow_fn(path[i - 1].x - path[i].x, 2);
        const double dy = pow_fn(path[i - 1].y - path[i].y, 2);
        s = s + sqrt_fn(dx + dy);
    }
    *len = s;
    return 0;
}

}  // extern "C"
