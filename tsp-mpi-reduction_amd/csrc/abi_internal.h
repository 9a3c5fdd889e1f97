// What the host files of the C ABI share (ctx.cpp, k1_launch.cpp,
// ragged_abi.cpp, cities_abi.cpp, the pipeline fronts of merge.hip): the
// workspace ordering rule, the host forms' round trip, the locked device
// forms, the range fan-out.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <thread>
#include <vector>

#include "ctx.h"
#include "ragged_plan.h"
#include "xfer.h"

namespace tspgpu {

// glibc's pow and sqrt really called (volatile pointers keep the compiler from
// folding pow(x, 2) to x*x): tspgpu_distance_matrix and the device build's
// fix-ups share them (k1_launch.cpp)
extern double (*volatile pow_fn)(double, double);
extern double (*volatile sqrt_fn)(double);

// ---- ctx.cpp ----
// Launches share the context's workspace (slots, push areas, parent words,
// ragged staging, fix-up list): before touching it on `stream`, wait for the
// previous launch if that ran on another stream; after the last launch, record
// the completion event the next one may wait for.  c->mu held.
int workspace_wait(tspgpu_ctx *c, hipStream_t stream);
int workspace_done(tspgpu_ctx *c, hipStream_t stream);

// ---- k1_launch.cpp ----
int check_n(int n, int strict);
int solve_device_locked(tspgpu_ctx *c, const void *d_dist, int n, int nblocks, void *d_cost, int32_t *d_tour,
                        hipStream_t stream, int vbytes);

// ---- ragged_abi.cpp ----
// The device work of one ragged call on `stream` (c->mu held).  The plan's
// source offsets are relative to d_dist + rebase elements (the host form
// uploads the covering extent only).  Nothing is waited for.
int ragged_locked(tspgpu_ctx *c, const void *d_dist, int vbytes, RaggedPlan &plan, int64_t rebase, void *d_cost,
                  int32_t *d_tour, int tour_stride, int32_t *d_status, hipStream_t stream);

// ---- cities_abi.cpp ----
// The call-level checks of the city forms, before the context is touched; 1:
// nothing to do (nblocks == 0).  Uniform (ragged false): n in [min_n,
// TSPGPU_MAX_CITIES], also for an empty batch, and within the context's limit
// for the solve forms (min_n >= 2).  Ragged: every ns[b] in [min_n,
// TSPGPU_MAX_CITIES]: the packed layout is undefined otherwise.  -> *max_n,
// *ncities.
int cities_args(const tspgpu_ctx *c, const void *cities, int n, const int32_t *ns, bool ragged, int nblocks,
                int min_n, int *max_n, int64_t *ncities);

// The matrices of nblocks blocks into d_dist on `stream` (c->mu held): n
// cities each, or, with ns (a host array, every entry in [1, 20]), packed
// ragged blocks of ns[b] cities (those above skip_above are not built).
// Synchronises the stream once per build pass; the patch and finish kernels
// are left running.
int cities_build_locked(tspgpu_ctx *c, const tspgpu_city *d_cities, int n, int nblocks, double *d_dist,
                        hipStream_t stream, const int32_t *ns = nullptr, int skip_above = TSPGPU_MAX_CITIES);

// ---- two_opt_abi.cpp ----
// What the 2-opt and Or-opt stages share (or_opt_abi.cpp): d_to_words holds
// the bounds and, behind them, a pass's candidate counter.
constexpr size_t kToCountAt = 64;
constexpr size_t kToWordsBytes = 128;
// The start of either stage on `stream` (c->mu held): the d_to_* buffers and
// the events reserved for L cities, the workspace waited for, d_path ->
// px, py, ord = pos = identity, the coordinates validated (-EINVAL, -ERANGE)
// and, from L = 4 up, the grid of *g by *g cells built and d_path copied to
// d_to_in; ev_to[0] and ev_to[1] stand around it all.  The bounds have been
// waited for, the grid kernels are left running.
int two_opt_state_locked(tspgpu_ctx *c, const tspgpu_city *d_path, int L, hipStream_t stream, int *g);
// *sum += the milliseconds between two recorded events that have passed
int two_opt_add_ms(double *sum, hipEvent_t from, hipEvent_t to);

// One buffer of a host form: reserved, then copied to or from `host`
struct HostCopy {
    DevBuf<char> *buf;
    void *host;
    size_t bytes;
};

// The round trip of a host form on the context's stream (c->mu held, the
// device set): reserve the buffers, upload, run() the locked device form,
// download, synchronise.  A failing run() is synchronised too: the caller's
// input may go once this returns.
template <typename Run>
int host_round_trip(tspgpu_ctx *c, HostCopy up, Run run, std::initializer_list<HostCopy> down)
{
    int rc = dev_reserve(*up.buf, up.bytes);
    for (const HostCopy &d : down)
        if (!rc) rc = dev_reserve(*d.buf, d.bytes);
    if (rc) return rc;
    hipError_t e = xcopy_async(up.buf->p, up.host, up.bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_err(e);
    if ((rc = run())) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    for (const HostCopy &d : down)
        if (e == hipSuccess) e = xcopy_async(d.host, d.buf->p, d.bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_err(e);
}

// fn(begin, end) over [0, count) split at count * t / nt, on up to
// nthreads_max host threads; one call below min_count
template <typename Fn>
void parallel_ranges(size_t count, unsigned nthreads_max, size_t min_count, Fn fn)
{
    size_t nt = std::min(nthreads_max, std::max(1u, std::thread::hardware_concurrency()));
    if (count < min_count) nt = 1;
    if (nt > count) nt = count > 0 ? count : 1;
    if (nt <= 1) {
        fn((size_t)0, count);
        return;
    }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back(fn, count * t / nt, count * (t + 1) / nt);
    for (auto &x : th) x.join();
}

}  // namespace tspgpu
