// C-ABI of libtspgpu (include/tspgpu.h): ragged batches —
// blocks of different sizes in one call, each validated on the device.  Host
// plan (ragged_plan.h) -> gather + validate (ragged.hip) -> one unchanged K1
// launch per size bucket -> scatter.
#include "tspgpu.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <mutex>

#include "abi_internal.h"
#include "ragged.h"

using namespace tspgpu;

namespace {

int ragged_vbytes(int dtype) { return dtype == TSPGPU_F64 ? 8 : (dtype == TSPGPU_I32 ? 4 : 0); }

// the call-level checks and the plan; 1: nothing to do (nblocks == 0)
int ragged_prepare(const tspgpu_ctx *c, const void *dist, int dtype, const int64_t *offset, const int32_t *n,
                   int nblocks, const void *cost, const void *tour, int tour_stride, const void *status,
                   RaggedPlan *plan)
{
    if (!c || nblocks < 0 || !ragged_vbytes(dtype)) return -EINVAL;
    if (nblocks == 0) return 1;
    if (!dist || !offset || !n || !cost || !tour || !status) return -EINVAL;
    const int rc = ragged_plan(n, offset, nblocks, c->strict, ragged_vbytes(dtype), plan);
    if (rc) return rc;
    if (tour_stride < plan->max_n + 1) return -EINVAL;
    return 0;
}

}  // namespace

int tspgpu::ragged_locked(tspgpu_ctx *c, const void *d_dist, int vbytes, RaggedPlan &plan, int64_t rebase,
                          void *d_cost, int32_t *d_tour, int tour_stride, int32_t *d_status, hipStream_t stream)
{
    const int nblocks = plan.nblocks;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    int rc = 0;
    const size_t desc_bytes = (size_t)nblocks * sizeof(RaggedDesc);
    if ((rc = dev_reserve(c->d_rg_dist, (size_t)plan.dist_elems * vbytes))) return rc;
    if ((rc = dev_reserve(c->d_rg_cost, (size_t)plan.cost_elems * vbytes))) return rc;
    if ((rc = dev_reserve(c->d_rg_tour, (size_t)plan.tour_elems * sizeof(int32_t)))) return rc;
    if ((rc = dev_reserve(c->d_rg_status, (size_t)nblocks * sizeof(int32_t)))) return rc;
    void *h = nullptr;
    if ((rc = c->rg_desc.begin(desc_bytes, &h))) return rc;
    RaggedDesc *hd = static_cast<RaggedDesc *>(h);
    for (int b = 0; b < nblocks; ++b) {
        hd[b] = plan.desc[b];
        if (!hd[b].pre) hd[b].src -= rebase;
    }
    // the staging buffers are the context's: under the workspace ordering rule
    if ((rc = workspace_wait(c, stream))) return rc;
    if ((rc = c->rg_desc.enqueue(desc_bytes, stream))) return rc;
    const RaggedDesc *dd = static_cast<const RaggedDesc *>(c->rg_desc.dev.p);
    hipError_t e = launch_ragged_gather(vbytes, d_dist, dd, nblocks, c->d_rg_dist, c->d_rg_status, stream);
    if (e != hipSuccess) return hip_err(e);
    for (int k = kRaggedMinN; k <= kRaggedMaxN; ++k) {
        if (!plan.count[k]) continue;
        rc = solve_device_locked(c, c->d_rg_dist + (size_t)plan.dist_base[k] * vbytes, k, plan.count[k],
                                 c->d_rg_cost + (size_t)plan.cost_base[k] * vbytes, c->d_rg_tour + plan.tour_base[k],
                                 stream, vbytes);
        if (rc) return rc;
    }
    e = launch_ragged_scatter(vbytes, dd, c->d_rg_status, nblocks, c->d_rg_cost, c->d_rg_tour, d_cost, d_tour,
                              tour_stride, d_status, stream);
    if (e != hipSuccess) return hip_err(e);
    return workspace_done(c, stream);
}

extern "C" {

int tspgpu_solve_ragged_device(tspgpu_ctx *c, const void *d_dist, int dtype, const int64_t *offset, const int32_t *n,
                               int nblocks, void *d_cost, int32_t *d_tour, int tour_stride, int32_t *d_status,
                               void *hip_stream)
{
    RaggedPlan plan;
    const int rc = ragged_prepare(c, d_dist, dtype, offset, n, nblocks, d_cost, d_tour, tour_stride, d_status, &plan);
    if (rc) return rc < 0 ? rc : 0;
    std::lock_guard<std::mutex> g(c->mu);
    return ragged_locked(c, d_dist, ragged_vbytes(dtype), plan, 0, d_cost, d_tour, tour_stride, d_status,
                         (hipStream_t)hip_stream);
}

int tspgpu_solve_ragged(tspgpu_ctx *c, const void *dist, int dtype, const int64_t *offset, const int32_t *n,
                        int nblocks, void *cost_out, int32_t *tour_out, int tour_stride, int32_t *status_out)
{
    RaggedPlan plan;
    int rc = ragged_prepare(c, dist, dtype, offset, n, nblocks, cost_out, tour_out, tour_stride, status_out, &plan);
    if (rc) return rc < 0 ? rc : 0;
    const int vbytes = ragged_vbytes(dtype);
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    // the covering extent of the in-range blocks in one copy (gaps travel too)
    const void *src = static_cast<const char *>(dist) + (size_t)plan.ext_lo * vbytes;
    auto run = [&] {
        return ragged_locked(c, c->d_dist, vbytes, plan, plan.ext_lo, c->d_cost, reinterpret_cast<int32_t *>(c->d_tour.p),
                             tour_stride, reinterpret_cast<int32_t *>(c->d_rg_ostatus.p), c->stream);
    };
    return host_round_trip(c, {&c->d_dist, const_cast<void *>(src), (size_t)(plan.ext_hi - plan.ext_lo) * vbytes}, run,
                           {{&c->d_cost, cost_out, (size_t)nblocks * vbytes},
                            {&c->d_tour, tour_out, (size_t)nblocks * tour_stride * sizeof(int32_t)},
                            {&c->d_rg_ostatus, status_out, (size_t)nblocks * sizeof(int32_t)}});
}

}  // extern "C"
