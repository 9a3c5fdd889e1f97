// C-ABI of libtspgpu (include/tspgpu.h): Or-opt with a neighbour grid on a
// path.  One call: the 2-opt stage's start (bounds, validation,
// the grid, once: two_opt_state_locked) -> per pass: search, the compact
// candidate list comes down, the host selects (or_opt_plan.h), the accepted
// moves go up, stage + commit -> emit.  The host selects for 2-opt's reason:
// the greedy acceptance is sequential in the sorted order, and everything a
// selection needs is 24 bytes per candidate.
#include "tspgpu.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <chrono>
#include <cstring>
#include <mutex>

#include "abi_internal.h"
#include "or_opt.h"
#include "or_opt_plan.h"

using namespace tspgpu;

namespace {

// the call-level checks of both forms
int or_opt_args(const tspgpu_ctx *c, const void *path, int L, int ring, int max_seg, int max_passes)
{
    if (!c || !path || L < 1 || (int64_t)L > kTwoOptMaxL) return -EINVAL;
    if (ring < 1 || ring > kTwoOptMaxRing || max_seg < 1 || max_seg > kOrOptMaxSeg || max_passes < 1) return -EINVAL;
    return 0;
}

// at most L / 3 disjoint moves (a range has three edges or more): lo, hi, how, prefix
size_t acc_stride(int L) { return (size_t)L / 3 + 2; }

int or_opt_reserve(tspgpu_ctx *c, int L)
{
    const size_t n = (size_t)L, acc = 4 * acc_stride(L) * sizeof(int32_t);
    int rc = 0;
    if ((rc = dev_reserve(c->d_oo_cand, n * sizeof(OrOptCand)))) return rc;
    if ((rc = dev_reserve(c->d_oo_acc, acc))) return rc;
    if ((rc = dev_reserve(c->d_oo_ord, n * sizeof(int32_t)))) return rc;
    if ((rc = dev_reserve(c->d_oo_px, n * sizeof(double)))) return rc;
    if ((rc = dev_reserve(c->d_oo_py, n * sizeof(double)))) return rc;
    if ((rc = pinned_reserve(c->h_oo_cand, n * sizeof(OrOptCand)))) return rc;
    return pinned_reserve(c->h_oo_acc, acc);
}

// The whole call on `stream` (c->mu held): synchronous.  d_path is written by
// the emit kernel alone, after every check has passed.
int or_opt_locked(tspgpu_ctx *c, tspgpu_city *d_path, int L, int ring, int max_seg, int max_passes,
                  tspgpu_or_opt_stats *st, hipStream_t stream)
{
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    // (reserved in front of the first kernel: growing a buffer may wait for the device)
    int rc = or_opt_reserve(c, L);
    if (rc) return rc;
    int g = 0;
    rc = two_opt_state_locked(c, d_path, L, stream, &g);
    if (rc || L < 4) return rc;  // L < 4: no legal move
    uint32_t *d_count = reinterpret_cast<uint32_t *>(c->d_to_words.p + kToCountAt);
    uint32_t *h_count = reinterpret_cast<uint32_t *>(c->h_to_words.p + kToCountAt);
    OrOptCand *d_cand = reinterpret_cast<OrOptCand *>(c->d_oo_cand.p);
    OrOptCand *h_cand = reinterpret_cast<OrOptCand *>(c->h_oo_cand.p);
    const size_t stride = acc_stride(L);
    int32_t *h_lo = c->h_oo_acc.p, *h_hi = h_lo + stride, *h_how = h_hi + stride, *h_prefix = h_how + stride;
    int32_t *d_lo = c->d_oo_acc.p, *d_hi = d_lo + stride, *d_how = d_hi + stride, *d_prefix = d_how + stride;
    hipError_t e = hipSuccess;
    bool grid_timed = false;
    for (;;) {
        e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[2], stream);
        if (e == hipSuccess)
            e = launch_or_opt_search(L, g, ring, max_seg, c->d_to_ord, c->d_to_pos, c->d_to_px, c->d_to_py,
                                     c->d_to_cell, c->d_to_start, c->d_to_cx, c->d_to_cy, c->d_to_city, d_cand,
                                     d_count, stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[3], stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_err(e);
        if (!grid_timed && (rc = two_opt_add_ms(&st->grid_ms, c->ev_to[0], c->ev_to[1]))) return rc;
        grid_timed = true;
        if ((rc = two_opt_add_ms(&st->search_ms, c->ev_to[2], c->ev_to[3]))) return rc;
        const int64_t n = *h_count;
        if (n > (int64_t)L - 2) return -EIO;  // more candidates than positions: the list is not ours
        if (n > 0) {
            e = hipMemcpyAsync(h_cand, d_cand, (size_t)n * sizeof(OrOptCand), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return hip_err(e);
        }
        const auto t0 = std::chrono::steady_clock::now();
        // (every candidate is checked before one is accepted, and checked ranges of three edges
        // or more that are disjoint inside L - 1 edges number L / 3 at the most: the lists hold them)
        const int64_t moves = or_opt_select(h_cand, n, L, max_seg, h_lo, h_hi, h_how, h_prefix, &st->gain);
        st->select_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (moves < 0 || moves > L / 3) return -EIO;  // a candidate outside the contract: nothing is applied
        st->passes += 1;
        st->candidates += n;
        st->moves += moves;
        if (moves == 0) break;
        const size_t mb = (size_t)moves * sizeof(int32_t);
        e = hipMemcpyAsync(d_lo, h_lo, mb, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_hi, h_hi, mb, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_how, h_how, mb, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_prefix, h_prefix, mb + sizeof(int32_t), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[4], stream);
        if (e == hipSuccess)
            e = launch_or_opt_apply((int)moves, d_lo, d_hi, d_how, d_prefix, h_prefix[moves], L, c->d_to_ord,
                                    c->d_to_pos, c->d_to_px, c->d_to_py, c->d_oo_ord, c->d_oo_px, c->d_oo_py, stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[5], stream);
        // (the next selection writes the pinned lists again: the uploads must have read them)
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_err(e);
        if ((rc = two_opt_add_ms(&st->apply_ms, c->ev_to[4], c->ev_to[5]))) return rc;
        if (st->passes == max_passes) break;
    }
    if (st->moves > 0) {
        e = launch_two_opt_emit(reinterpret_cast<const tspgpu_city *>(c->d_to_in.p), c->d_to_ord, L, d_path, stream);
        if (e != hipSuccess) return hip_err(e);
    }
    if ((rc = workspace_done(c, stream))) return rc;
    return hip_err(hipStreamSynchronize(stream));
}

}  // namespace

extern "C" {

int tspgpu_or_opt_path_device(tspgpu_ctx *c, tspgpu_city *d_path, int L, int ring, int max_seg, int max_passes,
                              tspgpu_or_opt_stats *stats, void *hip_stream)
{
    const int rc = or_opt_args(c, d_path, L, ring, max_seg, max_passes);
    if (rc) return rc;
    tspgpu_or_opt_stats st;
    std::memset(&st, 0, sizeof st);
    int out = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        out = or_opt_locked(c, d_path, L, ring, max_seg, max_passes, &st, (hipStream_t)hip_stream);
    }
    if (stats && !out) *stats = st;
    return out;
}

int tspgpu_or_opt_path(tspgpu_ctx *c, const tspgpu_city *path, int L, int ring, int max_seg, int max_passes,
                       tspgpu_city *path_out, tspgpu_or_opt_stats *stats)
{
    const int rc = or_opt_args(c, path, L, ring, max_seg, max_passes);
    if (rc) return rc;
    if (!path_out) return -EINVAL;
    tspgpu_or_opt_stats st;
    std::memset(&st, 0, sizeof st);
    int out = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
        const size_t bytes = (size_t)L * sizeof(tspgpu_city);
        auto run = [&] {
            return or_opt_locked(c, reinterpret_cast<tspgpu_city *>(c->d_to_path.p), L, ring, max_seg, max_passes, &st,
                                 c->stream);
        };
        out = host_round_trip(c, {&c->d_to_path, const_cast<tspgpu_city *>(path), bytes}, run,
                              {{&c->d_to_path, path_out, bytes}});
    }
    if (stats && !out) *stats = st;
    return out;
}

}  // extern "C"
