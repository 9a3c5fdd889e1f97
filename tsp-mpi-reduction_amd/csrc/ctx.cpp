// C-ABI of libtspgpu (include/tspgpu.h): the context and what hangs off it —
// create / destroy, streams, device memory and copies, timers, device
// information — and the small pure functions.
#include "tspgpu.h"
#include "tuning.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <mutex>
#include <new>

#include "abi_internal.h"

using namespace tspgpu;

int tspgpu::workspace_wait(tspgpu_ctx *c, hipStream_t stream)
{
    if (!c->k1_launched || stream == c->k1_last_stream) return 0;
    return hip_err(hipStreamWaitEvent(stream, c->ev_k1_done, 0));
}

int tspgpu::workspace_done(tspgpu_ctx *c, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    if (!c->ev_k1_done) e = hipEventCreateWithFlags(&c->ev_k1_done.p, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(c->ev_k1_done, stream);
    if (e != hipSuccess) return hip_err(e);
    c->k1_last_stream = stream;
    c->k1_launched = true;
    return 0;
}

extern "C" {

int tspgpu_version(void) { return TSPGPU_VERSION; }

const char *tspgpu_strerror(int code)
{
    switch (code) {
    case 0: return "success";
    case -EINVAL: return "invalid argument";
    case -ERANGE: return "tour costs reach INT_MAX (reference behaviour undefined)";
    case -ENODEV: return "no usable HIP device";
    case -ENOMEM: return "device allocation failed";
    case -EIO: return "HIP runtime or kernel launch failure";
    case -EDEADLK: return "the reference's mergeBlocks would never terminate for these paths";
    case -EOVERFLOW: return "too many tied optimal tours to enumerate above K1-wide's 31 cities";
    case -ENOSPC: return "output buffer too small";
    default: return "unknown error";
    }
}

int tspgpu_tour_length(int n) { return n == 2 ? 2 : n + 1; }

double tspgpu_relaxations_per_block(int n)
{
    const double N = n - 1;
    return N * (N - 1) * std::ldexp(1.0, n - 3);
}

double tspgpu_table_bytes_per_block(int n)
{
    const int N = n - 1;
    return 2.0 * 8.0 * N * std::ldexp(1.0, N - 1);
}

int tspgpu_ctx_create(const tspgpu_opts *opts, tspgpu_ctx **out)
{
    if (!out) return -EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -ENODEV;
    auto *c = new (std::nothrow) tspgpu_ctx();
    if (!c) return -ENOMEM;
    int dev = opts ? opts->device : -1;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= ndev) {
        delete c;
        return -ENODEV;
    }
    c->device = dev;
    c->strict = opts ? opts->strict : 0;
    c->slots_opt = opts ? opts->slots : 0;
    if (hipSetDevice(dev) != hipSuccess) {
        delete c;
        return -ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
        if (prop.multiProcessorCount > 0) c->cu_count = prop.multiProcessorCount;
        char nm[128] = {0};
        if (hipDeviceGetName(nm, sizeof nm, dev) != hipSuccess || !nm[0]) std::snprintf(nm, sizeof nm, "%s", prop.name);
        std::snprintf(c->name, sizeof c->name, "%s (%s, %d CUs)", nm[0] ? nm : "AMD GPU", prop.gcnArchName,
                      prop.multiProcessorCount);
    }
    // tuning knobs for experiments and tests (tuning.h; the defaults are the measured best)
    double kv = 0.0;
    if (tspgpu::tuned("THREADS", &kv)) c->threads = (int)kv;
    if (tspgpu::tuned("LDS_TABLE_MAX_N", &kv)) c->lds_table_max_n = (int)kv < kLdsTableMaxN ? (int)kv : kLdsTableMaxN;
    if (tspgpu::tuned("K1", &kv)) {
        // below 4: the compact layer pass (2); 4, 5 as given; above: 6
        const int v = (int)kv;
        c->variant = v >= 6 ? 6 : (v >= 4 ? v : 2);
    }
    if (tspgpu::tuned("TILED_CFG", &kv)) c->tiled_cfg = (int)kv;
    if (tspgpu::tuned("K1_CHUNK", &kv) && kv >= 1.0) c->k1_chunk = kv < 65536.0 ? (int)kv : 65536;
    if (tspgpu::tuned("WG_PER_CU", &kv)) c->wg_per_cu = kv > 0 ? (int)kv : 0;
    if (hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return -EIO;
    }
    *out = c;
    return 0;
}

int tspgpu_ctx_destroy(tspgpu_ctx *c)
{
    if (!c) return 0;
    {
        // searches still alive keep the context: the last one's destroy
        // releases it (ctx.h "Lifetime")
        std::lock_guard<std::mutex> g(c->mu);
        c->closing = true;
        if (c->live_searches > 0) return 0;
    }
    tspgpu_ctx_release(c);
    return 0;
}

}  // extern "C"

void tspgpu_ctx_release(tspgpu_ctx *c)
{
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;  // (every member frees itself, the stream last: ctx.h)
}

extern "C" {

int tspgpu_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int tspgpu_device_alloc(tspgpu_ctx *c, size_t bytes, void **ptr)
{
    if (!c || !ptr) return -EINVAL;
    *ptr = nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    return hip_err(hipMalloc(ptr, bytes ? bytes : 1));
}

int tspgpu_device_free(tspgpu_ctx *c, void *ptr)
{
    if (!c) return -EINVAL;
    if (!ptr) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    return hip_err(hipFree(ptr));
}

static int copy_sync(tspgpu_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (!c || (bytes && (!dst || !src))) return -EINVAL;
    if (!bytes) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    hipError_t e = xcopy_async(dst, src, bytes, kind, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_err(e);
}

int tspgpu_memcpy_htod(tspgpu_ctx *c, void *dst, const void *src, size_t bytes)
{
    return copy_sync(c, dst, src, bytes, hipMemcpyHostToDevice);
}

int tspgpu_memcpy_dtoh(tspgpu_ctx *c, void *dst, const void *src, size_t bytes)
{
    return copy_sync(c, dst, src, bytes, hipMemcpyDeviceToHost);
}

void *tspgpu_stream(tspgpu_ctx *c) { return c ? (void *)c->stream : nullptr; }

int tspgpu_stream_create(tspgpu_ctx *c, void **stream)
{
    if (!c || !stream) return -EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    *stream = e == hipSuccess ? (void *)s : nullptr;
    return hip_err(e);
}

int tspgpu_stream_destroy(tspgpu_ctx *c, void *stream)
{
    if (!c) return -EINVAL;
    if (!stream) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    std::lock_guard<std::mutex> g(c->mu);
    // (a descriptor upload may sit on this stream: let it finish first)
    c->rg_desc.drain();
    c->bd_desc.drain();
    // drained first: a pinned transfer slot whose last copy ran here is taken
    // again once its event can no longer be queried (xfer.hip HipSlots::done)
    (void)hipStreamSynchronize((hipStream_t)stream);
    if (c->k1_last_stream == (hipStream_t)stream) {
        // the next launch must not wait on an event of a destroyed stream's queue: forget it
        c->k1_launched = false;
        c->k1_last_stream = nullptr;
    }
    return hip_err(hipStreamDestroy((hipStream_t)stream));
}

int tspgpu_stream_synchronize(tspgpu_ctx *c, void *stream)
{
    if (!c) return -EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    return hip_err(hipStreamSynchronize((hipStream_t)stream));
}

int tspgpu_synchronize(tspgpu_ctx *c)
{
    if (!c) return -EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    return hip_err(hipStreamSynchronize(c->stream));
}

int tspgpu_timer_start(tspgpu_ctx *c)
{
    if (!c) return -EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    hipError_t e = hipSuccess;
    if (!c->ev_start) e = hipEventCreate(&c->ev_start.p);
    if (e == hipSuccess && !c->ev_stop) e = hipEventCreate(&c->ev_stop.p);
    if (e == hipSuccess) e = hipEventRecord(c->ev_start, c->stream);
    return hip_err(e);
}

int tspgpu_timer_stop(tspgpu_ctx *c, float *ms)
{
    if (!c || !ms || !c->ev_start) return -EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    hipError_t e = hipEventRecord(c->ev_stop, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(c->ev_stop);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, c->ev_start, c->ev_stop);
    return hip_err(e);
}

int tspgpu_device_info(const tspgpu_ctx *c, int *cu_count, char *name, int namecap)
{
    if (!c) return -EINVAL;
    if (cu_count) *cu_count = c->cu_count;
    if (name && namecap > 0) std::snprintf(name, (size_t)namecap, "%s", c->name);
    return 0;
}

}  // extern "C"
