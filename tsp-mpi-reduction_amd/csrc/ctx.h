// Internal definition of the opaque tspgpu_ctx (include/tspgpu.h): one HIP
// device, one stream, the K1 tables/workspaces and the K2 search state cache.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <vector>

#include "heldkarp.h"
#include "hipbuf.h"
#include "tspgpu.h"

// a type-erased cache another file owns the type of; empty = nothing cached
using tspgpu_erased = std::unique_ptr<void, void (*)(void *)>;

struct tspgpu_ctx {
    // (members are used by ctx.cpp, k1_launch.cpp, ragged_abi.cpp,
    // cities_abi.cpp, refine_abi.cpp and two_opt_abi.cpp for K1 and the tour
    // stages, search_abi.cpp for K2, merge.hip for K3)
    // Every buffer, event and cache below frees itself (hipbuf.h).  The stream
    // comes first so that it is destroyed after them all.
    tspgpu::Stream stream;
    int device = 0;
    int strict = 0;
    int slots_opt = 0;
    int cu_count = 256;
    tspgpu::DevBuf<uint32_t> d_masks[tspgpu::kMaxN + 1];
    tspgpu::DevBuf<tspgpu::LayerInfo> d_info[tspgpu::kMaxN + 1];
    tspgpu::DevBuf<double> d_slots;
    // the host forms' input and outputs (host_round_trip; values of either type)
    tspgpu::DevBuf<char> d_dist, d_cost, d_tour;
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
    tspgpu::DevBuf<void> d_tinfo[16];    // TiledInfo per L (variant 6)
    tspgpu::DevBuf<void> d_subrows[16];  // SubRow table per L (variant 6)
    tspgpu::DevBuf<char> d_tslots;       // variant 6 slots (one per block of a launch)
    tspgpu::Event ev_start, ev_stop;
    // K1 workspace ordering across caller streams: the slots / push areas are
    // per context, so a launch on a stream other than the previous one waits
    // for the previous launch (event recorded after every K1 launch):
    // workspace_wait / workspace_done, abi_internal.h
    tspgpu::Event ev_k1_done;
    // variant-5/6 split timing (tspgpu_k1_split_timing): per chunk launched
    // since the last read, three events (before the forward kernel, between
    // it and the backtracking kernel, after that); read and reset by
    // tspgpu_k1_last_split_ms
    int split_timing = 0;
    std::vector<tspgpu::Event> ev_split;
    size_t split_used = 0;
    bool split_overflow = false;
    hipStream_t k1_last_stream = nullptr;
    bool k1_launched = false;
    // Ragged batches (tspgpu_solve_ragged*, ragged_plan.h): the staging
    // buckets K1 solves from and into, the per-block descriptors and statuses.
    // Per context like the K1 workspace and under the same ordering rule
    // (ev_k1_done is recorded behind the scatter kernel too).
    tspgpu::PinnedUpload rg_desc;
    tspgpu::DevBuf<char> d_rg_dist, d_rg_cost;
    tspgpu::DevBuf<int32_t> d_rg_tour, d_rg_status;
    tspgpu::DevBuf<char> d_rg_ostatus;  // the host form's status output (its cost / tour use d_cost / d_tour)
    // Device distance build (tspgpu_distance_matrix_device, cities.h): the
    // fix-up list (slots; operands, overwritten by the host's pow results),
    // its counter, the pinned buffers the operands come down to and the
    // results go up from, the matrices of the solve forms and the upload
    // form's cities.  Per context
    // and under the K1 ordering rule (ev_k1_done behind the finish kernel).
    tspgpu::DevBuf<int64_t> d_ct_slot;
    tspgpu::DevBuf<double> d_ct_dx;
    tspgpu::DevBuf<unsigned long long> d_ct_count;
    tspgpu::DevBuf<double> d_ct_dist;
    tspgpu::DevBuf<char> d_ct_cities;
    tspgpu::Pinned<double> h_ct_fix;
    tspgpu::Pinned<unsigned long long> h_ct_count;
    // the last build (tspgpu_cities_last_fixups, tspgpu_cities_last_phase_ms)
    unsigned long long ct_squares = 0, ct_flagged = 0;
    int ct_passes = 0;
    double ct_build_ms = 0.0, ct_pow_ms = 0.0;
    // Packed ragged city blocks (tspgpu_distance_matrix_ragged_device,
    // block_desc.h): the per-block descriptor table of the build and finish
    // kernels.  The device table is ordered like the fix-up list, behind
    // ev_k1_done.
    tspgpu::PinnedUpload bd_desc;
    // Fixed-end paths and the window refinement (refine_abi.cpp, DESIGN.md
    // §6d): the folded matrices K1 solves; a pass's packed windows, their
    // matrices, K1's answers, the identity costs, gains and replaced flags
    // with the pinned buffers these come down to; the host form's path; the
    // five events that time a pass.  Per context and under the K1 ordering
    // rule.
    tspgpu::DevBuf<char> d_rf_fold, d_rf_cities, d_rf_path;
    tspgpu::DevBuf<double> d_rf_dist, d_rf_cost, d_rf_old, d_rf_gain;
    tspgpu::DevBuf<int32_t> d_rf_tour, d_rf_status, d_rf_flag;
    tspgpu::Pinned<double> h_rf_gain;
    tspgpu::Pinned<int32_t> h_rf_flag, h_rf_status;
    tspgpu::Event ev_rf[5];
    // 2-opt with a neighbour grid (two_opt_abi.cpp): the host
    // form's path and the copy of the input the final order is gathered
    // from; the state by position (ord, pos, px, py); the grid (cell of a
    // city, the cells' starts and fill cursors, the scan's partial sums, the
    // cell-sorted x, y, city); a pass's candidates and accepted moves (i, j,
    // swap prefix) with their pinned twins; the bounds and the candidate
    // counter as one block of words; the six events that time the grid
    // build, a search and an apply.  Per context and under the K1 ordering
    // rule.
    tspgpu::DevBuf<char> d_to_path, d_to_in, d_to_cand, d_to_words;
    tspgpu::DevBuf<int32_t> d_to_ord, d_to_pos, d_to_cell, d_to_start, d_to_cursor, d_to_sums, d_to_city, d_to_acc;
    tspgpu::DevBuf<double> d_to_px, d_to_py, d_to_cx, d_to_cy;
    tspgpu::Pinned<char> h_to_cand, h_to_words;
    tspgpu::Pinned<int32_t> h_to_acc;
    tspgpu::Event ev_to[6];
    // Or-opt with a neighbour grid (or_opt_abi.cpp) runs on
    // the 2-opt stage's path, state, grid, words and events, and adds a
    // pass's candidates and accepted moves (lo, hi, how, length prefix) with
    // their pinned twins and the scratch a rotation is staged in (ord, px,
    // py of the rotated positions).  Per context and under the K1 ordering
    // rule.
    tspgpu::DevBuf<char> d_oo_cand;
    tspgpu::DevBuf<int32_t> d_oo_acc, d_oo_ord;
    tspgpu::DevBuf<double> d_oo_px, d_oo_py;
    tspgpu::Pinned<char> h_oo_cand;
    tspgpu::Pinned<int32_t> h_oo_acc;
    // the last tspgpu_reduce_device's gather + summary + uniqueness kernels,
    // from HIP events (tspgpu_reduce_device_last_ms)
    double k3_gather_ms = 0.0;
    tspgpu::Event ev_k3_gather[2];  // created by the first tspgpu_reduce_device
    char name[256] = {0};
    std::mutex mu;
    // K1-wide per-context cache (buffers of the last (n, value type)), hkwide_impl.h
    tspgpu_erased wide_cache{nullptr, nullptr};
    int wide_last_dtype = -1;  // value type of the last K1-wide launch (tspgpu_wide_last_dtype)
    // K2 device buffers kept between searches (search_abi.cpp); empty while a
    // live search holds them
    tspgpu_erased search_pool{nullptr, nullptr};
    // Lifetime: every tspgpu_search holds a reference on its context (it uses
    // the stream, the device, the mutex and the pool).  tspgpu_ctx_destroy
    // with searches still alive only marks the context closing; the last
    // tspgpu_search_destroy then releases it.  Both under mu.
    int live_searches = 0;
    bool closing = false;
};

// drains the stream and deletes c, whose members free themselves (no live
// search may remain)
void tspgpu_ctx_release(tspgpu_ctx *c);
