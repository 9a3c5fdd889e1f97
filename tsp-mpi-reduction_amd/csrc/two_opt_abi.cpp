// C-ABI of libtspgpu (include/tspgpu.h): 2-opt with a neighbour grid on a
// path.  One call: bounds kernel -> the host validates the
// five values -> cells, scan, fill (the grid, once) -> per pass: search, the
// compact candidate list comes down, the host selects (two_opt_plan.h), the
// accepted moves go up, apply -> emit.  The host selects because the greedy
// acceptance is sequential in the sorted order; everything a selection needs
// is 16 bytes per candidate.
#include "tspgpu.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>

#include "abi_internal.h"
#include "two_opt.h"
#include "two_opt_plan.h"

using namespace tspgpu;

static_assert(sizeof(TwoOptBounds) <= kToCountAt, "the counter stands behind the bounds");

namespace {

// the call-level checks of both forms
int two_opt_args(const tspgpu_ctx *c, const void *path, int L, int ring, int max_passes)
{
    if (!c || !path || L < 1 || (int64_t)L > kTwoOptMaxL) return -EINVAL;
    if (ring < 1 || ring > kTwoOptMaxRing || max_passes < 1) return -EINVAL;
    return 0;
}

int two_opt_events(tspgpu_ctx *c)
{
    for (tspgpu::Event &ev : c->ev_to)
        if (!ev) {
            const hipError_t e = hipEventCreate(&ev.p);
            if (e != hipSuccess) return hip_err(e);
        }
    return 0;
}

int two_opt_reserve(tspgpu_ctx *c, int L, int cells)
{
    const size_t n = (size_t)L, i32 = sizeof(int32_t), f64 = sizeof(double);
    const size_t acc = (3 * (n / 3 + 1) + 1) * i32;  // at most L / 3 disjoint moves: i, j, prefix
    int rc = 0;
    if ((rc = dev_reserve(c->d_to_in, n * sizeof(tspgpu_city)))) return rc;
    if ((rc = dev_reserve(c->d_to_cand, n * sizeof(TwoOptCand)))) return rc;
    if ((rc = dev_reserve(c->d_to_words, kToWordsBytes))) return rc;
    if ((rc = dev_reserve(c->d_to_ord, n * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_pos, n * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_cell, n * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_start, ((size_t)cells + 1) * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_cursor, (size_t)cells * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_sums, ((size_t)cells / 1024 + 1) * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_city, n * i32))) return rc;
    if ((rc = dev_reserve(c->d_to_acc, acc))) return rc;
    if ((rc = dev_reserve(c->d_to_px, n * f64))) return rc;
    if ((rc = dev_reserve(c->d_to_py, n * f64))) return rc;
    if ((rc = dev_reserve(c->d_to_cx, n * f64))) return rc;
    if ((rc = dev_reserve(c->d_to_cy, n * f64))) return rc;
    if ((rc = pinned_reserve(c->h_to_cand, n * sizeof(TwoOptCand)))) return rc;
    if ((rc = pinned_reserve(c->h_to_words, kToWordsBytes))) return rc;
    if ((rc = pinned_reserve(c->h_to_acc, acc))) return rc;
    return two_opt_events(c);
}

}  // namespace

int tspgpu::two_opt_add_ms(double *sum, hipEvent_t from, hipEvent_t to)
{
    float ms = 0.0f;
    const hipError_t e = hipEventElapsedTime(&ms, from, to);
    if (e != hipSuccess) return hip_err(e);
    *sum += ms;
    return 0;
}

int tspgpu::two_opt_state_locked(tspgpu_ctx *c, const tspgpu_city *d_path, int L, hipStream_t stream, int *g_out)
{
    if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
    const int g = *g_out = two_opt_grid(L), cells = g * g;
    int rc = two_opt_reserve(c, L, cells);
    if (rc) return rc;
    // every buffer below is the context's: under the workspace ordering rule
    if ((rc = workspace_wait(c, stream))) return rc;
    TwoOptBounds *d_bounds = reinterpret_cast<TwoOptBounds *>(c->d_to_words.p);
    TwoOptBounds *h_bounds = reinterpret_cast<TwoOptBounds *>(c->h_to_words.p);

    // bounds + validation; the state starts as the identity order
    *h_bounds = two_opt_bounds_init();
    hipError_t e = hipEventRecord(c->ev_to[0], stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_bounds, h_bounds, sizeof(TwoOptBounds), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess)
        e = launch_two_opt_bounds(d_path, L, c->d_to_px, c->d_to_py, c->d_to_ord, c->d_to_pos, d_bounds, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_bounds, d_bounds, sizeof(TwoOptBounds), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return hip_err(e);
    if ((rc = workspace_done(c, stream))) return rc;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return hip_err(e);
    if (h_bounds->nonfinite) return -EINVAL;
    const double xmin = two_opt_decode(h_bounds->xmin), ymin = two_opt_decode(h_bounds->ymin);
    const double ex = two_opt_decode(h_bounds->xmax) - xmin, ey = two_opt_decode(h_bounds->ymax) - ymin;
    if (!std::isfinite(ex) || !std::isfinite(ey) || !std::isfinite(ex * ex + ey * ey)) return -ERANGE;
    if (L < 4) return 0;  // no legal move

    // the grid, once, and the copy of the input the final order is gathered from
    e = hipMemsetAsync(c->d_to_start, 0, ((size_t)cells + 1) * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_to_cursor, 0, (size_t)cells * sizeof(int32_t), stream);
    if (e == hipSuccess)
        e = launch_two_opt_cells(c->d_to_px, c->d_to_py, L, xmin, ex, ymin, ey, g, c->d_to_cell, c->d_to_start, stream);
    if (e == hipSuccess) e = launch_two_opt_scan(c->d_to_start, cells, L, c->d_to_start, c->d_to_sums, stream);
    if (e == hipSuccess)
        e = launch_two_opt_fill(c->d_to_px, c->d_to_py, c->d_to_cell, L, c->d_to_start, c->d_to_cursor, c->d_to_cx,
                                c->d_to_cy, c->d_to_city, stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->d_to_in, d_path, (size_t)L * sizeof(tspgpu_city), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(c->ev_to[1], stream);
    return hip_err(e);
}

namespace {

// The whole call on `stream` (c->mu held): synchronous.  d_path is written by
// the emit kernel alone, after every check has passed.
int two_opt_locked(tspgpu_ctx *c, tspgpu_city *d_path, int L, int ring, int max_passes, tspgpu_two_opt_stats *st,
                   hipStream_t stream)
{
    int g = 0;
    int rc = two_opt_state_locked(c, d_path, L, stream, &g);
    if (rc || L < 4) return rc;  // L < 4: no legal move
    uint32_t *d_count = reinterpret_cast<uint32_t *>(c->d_to_words.p + kToCountAt);
    uint32_t *h_count = reinterpret_cast<uint32_t *>(c->h_to_words.p + kToCountAt);
    TwoOptCand *d_cand = reinterpret_cast<TwoOptCand *>(c->d_to_cand.p);
    TwoOptCand *h_cand = reinterpret_cast<TwoOptCand *>(c->h_to_cand.p);
    hipError_t e = hipSuccess;

    int32_t *h_i = c->h_to_acc.p, *h_j = h_i + (L / 3 + 1), *h_prefix = h_j + (L / 3 + 1);
    int32_t *d_i = c->d_to_acc.p, *d_j = d_i + (L / 3 + 1), *d_prefix = d_j + (L / 3 + 1);
    bool grid_timed = false;
    for (;;) {
        e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[2], stream);
        if (e == hipSuccess)
            e = launch_two_opt_search(L, g, ring, c->d_to_ord, c->d_to_pos, c->d_to_px, c->d_to_py, c->d_to_cell,
                                      c->d_to_start, c->d_to_cx, c->d_to_cy, c->d_to_city, d_cand, d_count, stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[3], stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_err(e);
        if (!grid_timed && (rc = two_opt_add_ms(&st->grid_ms, c->ev_to[0], c->ev_to[1]))) return rc;
        grid_timed = true;
        if ((rc = two_opt_add_ms(&st->search_ms, c->ev_to[2], c->ev_to[3]))) return rc;
        const int64_t n = *h_count;
        if (n > (int64_t)L - 3) return -EIO;  // more candidates than positions: the list is not ours
        if (n > 0) {
            e = hipMemcpyAsync(h_cand, d_cand, (size_t)n * sizeof(TwoOptCand), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return hip_err(e);
        }
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t moves = two_opt_select(h_cand, n, L, h_i, h_j, h_prefix, &st->gain);
        st->select_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (moves < 0 || moves > L / 3) return -EIO;  // a candidate outside the path: nothing is applied
        st->passes += 1;
        st->candidates += n;
        st->moves += moves;
        if (moves == 0) break;
        const size_t mb = (size_t)moves * sizeof(int32_t);
        e = hipMemcpyAsync(d_i, h_i, mb, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_j, h_j, mb, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_prefix, h_prefix, mb + sizeof(int32_t), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_to[4], stream);
        if (e == hipSuccess)
            e = launch_two_opt_apply((int)moves, d_i, d_j, d_prefix, h_prefix[moves], c->d_to_ord, c->d_to_pos,
                                     c->d_to_px, c->d_to_py, stream);
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

int tspgpu_two_opt_path_device(tspgpu_ctx *c, tspgpu_city *d_path, int L, int ring, int max_passes,
                               tspgpu_two_opt_stats *stats, void *hip_stream)
{
    const int rc = two_opt_args(c, d_path, L, ring, max_passes);
    if (rc) return rc;
    tspgpu_two_opt_stats st;
    std::memset(&st, 0, sizeof st);
    int out = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        out = two_opt_locked(c, d_path, L, ring, max_passes, &st, (hipStream_t)hip_stream);
    }
    if (stats && !out) *stats = st;
    return out;
}

int tspgpu_two_opt_path(tspgpu_ctx *c, const tspgpu_city *path, int L, int ring, int max_passes,
                        tspgpu_city *path_out, tspgpu_two_opt_stats *stats)
{
    const int rc = two_opt_args(c, path, L, ring, max_passes);
    if (rc) return rc;
    if (!path_out) return -EINVAL;
    tspgpu_two_opt_stats st;
    std::memset(&st, 0, sizeof st);
    int out = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (hipSetDevice(c->device) != hipSuccess) return -ENODEV;
        const size_t bytes = (size_t)L * sizeof(tspgpu_city);
        auto run = [&] {
            return two_opt_locked(c, reinterpret_cast<tspgpu_city *>(c->d_to_path.p), L, ring, max_passes, &st,
                                  c->stream);
        };
        out = host_round_trip(c, {&c->d_to_path, const_cast<tspgpu_city *>(path), bytes}, run,
                              {{&c->d_to_path, path_out, bytes}});
    }
    if (stats && !out) *stats = st;
    return out;
}

}  // extern "C"
