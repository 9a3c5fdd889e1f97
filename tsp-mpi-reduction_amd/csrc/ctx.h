// Internal definition of the opaque tspgpu_ctx (include/tspgpu.h): one HIP
// device, one stream, the K1 tables/workspaces and the K2 search state cache.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "heldkarp.h"
#include "tspgpu.h"

struct tspgpu_ctx {
    // (members are used by tspgpu.cpp for K1 and search_abi.cpp for K2)
    int device = 0;
    int strict = 0;
    int slots_opt = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    uint32_t *d_masks[tspgpu::kMaxN + 1] = {};
    tspgpu::LayerInfo *d_info[tspgpu::kMaxN + 1] = {};
    double *d_slots = nullptr;
    size_t slots_bytes = 0;
    double *d_dist = nullptr;
    size_t dist_bytes = 0;
    double *d_cost = nullptr;
    size_t cost_bytes = 0;
    int32_t *d_tour = nullptr;
    size_t tour_bytes = 0;
    int last_grid = 0;
    int last_variant = -1;
    int threads = 0;     // workgroup size of the global-table kernels; 0 = per-N default
    int wg_per_cu = 0;   // resident slots per CU (auto grid); 0 = per-N default
    int lds_table_max_n = tspgpu::kLdsTableDefaultMaxN;  // largest N whose whole table stays in LDS
    int variant = -1;    // K1 variant (-1: per-n default): 6 = sub-cube (hk_sub.h),
                         // 5 = what 6 falls back to where it has no configuration (the retired variant 5),
                         // 4 = 2 + ping-pong values + parent words,
                         // 2 = compact layer pass + next-row prefetch
    int tiled_cfg = -1;  // K1 variant 6 configuration id (k1_cfg.h); -1 = per-(n, type) default
    int k1_chunk = 65536;  // most blocks per variant-6 chunk (ensure_slots; knob K1_CHUNK for tests)
    void *d_tinfo[16] = {};        // TiledInfo per L (variant 6)
    void *d_subrows[16] = {};      // SubRow table per L (variant 6)
    char *d_tslots = nullptr;      // variant 6 slots (one per block of a launch)
    size_t tslots_bytes = 0;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // K1 workspace ordering across caller streams: the slots / push areas are
    // per context, so a launch on a stream other than the previous one waits
    // for the previous launch (event recorded after every K1 launch)
    hipEvent_t ev_k1_done = nullptr;
    // variant-5/6 split timing (tspgpu_k1_split_timing): per chunk launched
    // since the last read, three events (before the forward kernel, between
    // it and the backtracking kernel, after that); read and reset by
    // tspgpu_k1_last_split_ms
    int split_timing = 0;
    std::vector<hipEvent_t> ev_split;
    size_t split_used = 0;
    bool split_overflow = false;
    hipStream_t k1_last_stream = nullptr;
    bool k1_launched = false;
    // Ragged batches (tspgpu_solve_ragged*, ragged_plan.h): the staging
    // buckets K1 solves from and into, the per-block descriptors and statuses.
    // Per context like the K1 workspace and under the same ordering rule
    // (ev_k1_done is recorded behind the scatter kernel too).  The descriptors
    // are uploaded from a pinned buffer; ev_rg_desc fires when that copy has
    // read it, and the next ragged call waits for it before it writes there.
    void *d_rg_desc = nullptr;
    size_t rg_desc_bytes = 0;
    void *d_rg_dist = nullptr;
    size_t rg_dist_bytes = 0;
    void *d_rg_cost = nullptr;
    size_t rg_cost_bytes = 0;
    int32_t *d_rg_tour = nullptr;
    size_t rg_tour_bytes = 0;
    int32_t *d_rg_status = nullptr;
    size_t rg_status_bytes = 0;
    int32_t *d_rg_ostatus = nullptr;  // the host form's status output (its cost / tour use d_cost / d_tour)
    size_t rg_ostatus_bytes = 0;
    void *h_rg_desc = nullptr;        // pinned
    size_t h_rg_desc_bytes = 0;
    hipEvent_t ev_rg_desc = nullptr;
    bool rg_desc_pending = false;
    // Device distance build (tspgpu_distance_matrix_device, cities.h): the
    // fix-up list (slots; operands, overwritten by the host's pow results),
    // its counter, the pinned buffers the operands come down to and the
    // results go up from, the matrices of the solve forms and the upload
    // form's cities.  Per context
    // and under the K1 ordering rule (ev_k1_done behind the finish kernel).
    int64_t *d_ct_slot = nullptr;
    size_t ct_slot_bytes = 0;
    double *d_ct_dx = nullptr;
    size_t ct_dx_bytes = 0;
    unsigned long long *d_ct_count = nullptr;
    size_t ct_count_bytes = 0;
    double *d_ct_dist = nullptr;
    size_t ct_dist_bytes = 0;
    tspgpu_city *d_ct_cities = nullptr;
    size_t ct_cities_bytes = 0;
    double *h_ct_fix = nullptr;              // pinned
    size_t h_ct_fix_bytes = 0;
    unsigned long long *h_ct_count = nullptr;  // pinned
    // the last build (tspgpu_cities_last_fixups, tspgpu_cities_last_phase_ms)
    unsigned long long ct_squares = 0, ct_flagged = 0;
    int ct_passes = 0;
    double ct_build_ms = 0.0, ct_pow_ms = 0.0;
    // Packed ragged city blocks (tspgpu_distance_matrix_ragged_device,
    // block_desc.h): the per-block descriptor table of the build and finish
    // kernels, uploaded from a pinned buffer under the rule of h_rg_desc
    // (ev_bd_desc fires when the copy has read it; the next call waits for
    // that before it writes there).  The device table is ordered like the
    // fix-up list, behind ev_k1_done.
    void *d_bd_desc = nullptr;
    size_t bd_desc_bytes = 0;
    void *h_bd_desc = nullptr;  // pinned
    size_t h_bd_desc_bytes = 0;
    hipEvent_t ev_bd_desc = nullptr;
    bool bd_desc_pending = false;
    // the last tspgpu_reduce_device's gather + summary + uniqueness kernels,
    // from HIP events (tspgpu_reduce_device_last_ms)
    double k3_gather_ms = 0.0;
    hipEvent_t ev_k3_gather[2] = {nullptr, nullptr};  // created by the first tspgpu_reduce_device
    char name[256] = {0};
    std::mutex mu;
    // K1-wide per-context cache (buffers of the last (n, value type)), hkwide_impl.h
    void *wide_cache = nullptr;
    void (*wide_free)(void *) = nullptr;
    int wide_last_dtype = -1;  // value type of the last K1-wide launch (tspgpu_wide_last_dtype)
    // K2 device buffers kept between searches (search_abi.cpp); null while a
    // live search holds them
    void *search_pool = nullptr;
    void (*search_pool_free)(void *) = nullptr;
    // Lifetime: every tspgpu_search holds a reference on its context (it uses
    // the stream, the device, the mutex and the pool).  tspgpu_ctx_destroy
    // with searches still alive only marks the context closing; the last
    // tspgpu_search_destroy then releases it.  Both under mu.
    int live_searches = 0;
    bool closing = false;
};

// frees every resource of c and c itself (no live search may remain)
void tspgpu_ctx_release(tspgpu_ctx *c);
