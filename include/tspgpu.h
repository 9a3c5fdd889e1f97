/*
 * tspgpu — MI355X (gfx950) exact TSP block search behind a C ABI.
 *
 * Drop-in for the reference's per-block solver
 *     BlockSolution tsp(vector<City> cities)        (assignment2.h:56, tsp.cpp:405-509)
 * and its helper computeDistanceMatrix               (assignment2.h:184-200).
 * Results are bit-identical to the reference: the same FP64 optimal cost and
 * the same tour (the reference's first-strict-minimum tie rule, tsp.cpp:457-470,
 * 484-498).  Plain C types only; no HIP or torch types cross this boundary
 * (HIP streams are passed as void*).  See INTEGRATION.md for the C++/ctypes
 * bindings a maintainer of the reference would add.
 *
 * Return codes: 0 on success, otherwise a negative errno value
 *   -EINVAL  bad argument (n outside [2, TSPGPU_MAX_CITIES] (strict: 16), nblocks < 0,
 *            NULL pointer, non-finite or negative distance; -0.0 counts as
 *            negative: a minimum over zeros of both signs has no defined sign;
 *            (K3) a non-finite coordinate, see K3's coordinate domain below)
 *   -ERANGE  n * max(d) >= INT_MAX: the reference's INT_MAX sentinel
 *            (tsp.cpp:411,453) would leave its tour undefined
 *   -ENODEV  no HIP device / device ordinal out of range
 *   -ENOMEM  device allocation failed
 *   -EIO     a HIP runtime call or kernel launch failed; (K3) no swap cost below
 *            INT_MAX, see K3's coordinate domain below
 *   -EDEADLK (K3) the reference's mergeBlocks would never terminate for these paths
 *            (its rotation loop, tsp.cpp:236-239, looks for a city that is not there);
 *            promised, like every K3 answer, inside K3's coordinate domain below
 *   -ENOSPC  (K3) the merged tour is longer than path_cap (everything else was written)
 *   -EOVERFLOW (K2) more optimal tours than can be enumerated, n > 31
 *
 * K3's coordinate domain (tspgpu_merge, every tspgpu_reduce* and
 * tspgpu_pipeline* form).  The reference's pair, cost and path are promised
 * where
 *   (1) every coordinate is finite (else -EINVAL);
 *   (2) the square of every coordinate difference is zero or lies in
 *       [2^-900, 2^1000]: the device's dx*dx then neither underflows nor
 *       overflows against the host's pow (not checked);
 *   (3) the minimum swap cost of every merge is below INT_MAX, the value the
 *       reference's search starts from (above it the reference's own result
 *       is undefined; the call may return -EIO).
 * Sign, translation and power-of-two scale inside (2) are free.
 */
#ifndef TSPGPU_H
#define TSPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSPGPU_VERSION 100          /* 1.0.0 */
#define TSPGPU_MAX_CITIES 20        /* extension limit (N = n-1 <= 19) */
#define TSPGPU_REFERENCE_MAX_CITIES 16 /* tsp.cpp:289 rejects more */

/* Memory layout identical to the reference's City (assignment2.h:13-18):
 * int id at offset 0, double x at 8, double y at 16; 24 bytes. */
typedef struct
{
    int32_t id;
    double x;
    double y;
} tspgpu_city;

typedef struct
{
    int device;      /* HIP device ordinal; -1 = the calling thread's current device */
    int strict;      /* 1: accept n <= 16 only (the reference's cap, tsp.cpp:289) */
    int slots;       /* resident DP workspaces = persistent grid size of the global-table
                        layer kernels (11 cities and more); 0 = auto.  The LDS-table
                        kernels (up to 10 cities) keep no workspace and the large-batch
                        sub-cube kernel sizes its own grid: both ignore it. */
    int reserved[5]; /* must be zero */
} tspgpu_opts;

typedef struct tspgpu_ctx tspgpu_ctx;

int tspgpu_version(void);
const char *tspgpu_strerror(int code);

/* Length of the tour written per block: n+1 (0, t1..tN, 0), except the
 * reference's n==2 quirk [1,0] (tsp.cpp:483-502 with one inner city). */
int tspgpu_tour_length(int n);

/* computeDistanceMatrix (assignment2.h:184-200) on the host with glibc pow/sqrt,
 * bit-exact with the reference.  dist: nblocks*n*n row-major. */
int tspgpu_distance_matrix(const tspgpu_city *cities, int n, int nblocks, double *dist);

/* Host-side validation applied by the host-pointer entry points. */
int tspgpu_validate(const double *dist, int n, int nblocks, int strict);

int tspgpu_ctx_create(const tspgpu_opts *opts, tspgpu_ctx **out);
/* Destroy order is free: every tspgpu_search holds a reference on its
 * context, so destroying the context while searches are alive only marks it
 * closing (no new search may be created on it: -EINVAL) and the last
 * tspgpu_search_destroy releases it.  Searches never destroyed keep their
 * context (a leak, never a use-after-free). */
int tspgpu_ctx_destroy(tspgpu_ctx *ctx);

/* Batched replacement for tsp() on host buffers; synchronous.
 *   dist     nblocks*n*n doubles (host), from tspgpu_distance_matrix
 *   cost_out nblocks doubles: the block's tour cost (BlockSolution.cost)
 *   tour_out nblocks*(n+1) int32: local city indices of BlockSolution.path
 *            (tspgpu_tour_length(n) valid entries; the rest is -1) */
int tspgpu_solve_blocks(tspgpu_ctx *ctx, const double *dist, int n, int nblocks, double *cost_out,
                        int32_t *tour_out);

/* Same, from cities (distance matrix computed on the host, then solved;
 * tspgpu_solve_cities_upload below builds it on the device instead). */
int tspgpu_solve_cities(tspgpu_ctx *ctx, const tspgpu_city *cities, int n, int nblocks, double *cost_out,
                        int32_t *tour_out);

/* Device-pointer form, asynchronous on `hip_stream` (hipStream_t, NULL = default).
 * The caller guarantees the data satisfy tspgpu_validate (not re-checked).
 * d_dist/d_cost/d_tour are device pointers on the context's device.
 * Calls on one context may use different streams: they share the context's
 * DP workspace, so a launch on a stream other than the previous launch's
 * waits (hipStreamWaitEvent) for that launch first; use one context per
 * stream for concurrent batches. */
int tspgpu_solve_blocks_device(tspgpu_ctx *ctx, const double *d_dist, int n, int nblocks, double *d_cost,
                               int32_t *d_tour, void *hip_stream);

/* Integer-weight extension (TSPLIB-style rounded distances; no reference
 * counterpart — the reference computes f64 Euclidean distances only): the same
 * DP, tie rule and tour layout on int32 distances.  Results equal
 * tspgpu_solve_blocks on the same matrix converted to double (every partial
 * sum is an exact integer below 2^31); the table and its HBM traffic are half
 * the size.  Validation: d >= 0 and n * max(d) < INT_MAX (else -ERANGE). */
int tspgpu_validate_i32(const int32_t *dist, int n, int nblocks, int strict);
int tspgpu_solve_blocks_i32(tspgpu_ctx *ctx, const int32_t *dist, int n, int nblocks, int32_t *cost_out,
                            int32_t *tour_out);
int tspgpu_solve_blocks_i32_device(tspgpu_ctx *ctx, const int32_t *d_dist, int n, int nblocks, int32_t *d_cost,
                                   int32_t *d_tour, void *hip_stream);

/* ---------------------------------------------------------------------------
 * Ragged batches: blocks of DIFFERENT city counts in one call, every block
 * validated on the device, one status per block.  block b is the n[b] x n[b]
 * row-major matrix at element offset[b] of the distance array (elements of
 * dtype: TSPGPU_F64 doubles or TSPGPU_I32 int32).  Offsets need no alignment
 * beyond the element's, and may overlap, repeat and come in any order.
 *
 * One device pass validates every block while it gathers it into a
 * contiguous bucket per size; every non-empty bucket is then one ordinary K1
 * launch, in ascending n (the kernels and dispatch of tspgpu_solve_blocks,
 * unchanged); a second pass writes the answers back in caller order.
 *
 * The contract.  The call returns 0 however many blocks are bad; status[b]
 * says which.
 *   status[b] == 0: cost[b] (dtype's type) and tour row b equal, bit for bit,
 *     what tspgpu_solve_blocks / tspgpu_solve_blocks_i32 returns for that
 *     matrix alone — hence tsp()'s.  Row b of the tour array starts at
 *     b * tour_stride: tspgpu_tour_length(n[b]) entries, then -1 up to
 *     tour_stride.
 *   otherwise status[b] equals tspgpu_validate(matrix, n[b], 1, strict) /
 *     tspgpu_validate_i32(...): -EINVAL (n[b] outside [2, 20] (strict: 16),
 *     offset[b] < 0 — such a block's matrix is never read — or a negative,
 *     non-finite or -0.0 element), -ERANGE (n * max(d) >= INT_MAX); or it is
 *     -EIO (the kernel found no tour; never seen on validated data).  Its
 *     cost is NaN (f64) or -1 (int32) and its whole tour row is -1.  A bad
 *     block costs only itself: its neighbours are solved.
 * Called with one n for every block this is the validated form of
 * tspgpu_solve_blocks_device.
 *
 * Call-level errors (nothing is launched, no output is written): -EINVAL for
 * a NULL context, a NULL pointer with nblocks > 0, nblocks < 0, an unknown
 * dtype, or tour_stride < (largest in-range n[b]) + 1; -ENOMEM, -ENODEV, -EIO
 * as elsewhere.  nblocks == 0 returns 0.
 *
 * After a ragged call tspgpu_last_variant / tspgpu_last_grid report the LAST
 * bucket launched, i.e. the one of the largest in-range n (unchanged when no
 * block was in range).
 * ------------------------------------------------------------------------- */
#define TSPGPU_F64 0
#define TSPGPU_I32 1
/* Device-pointer form, asynchronous on `hip_stream`.  d_dist, d_cost, d_tour
 * (nblocks * tour_stride int32) and d_status (nblocks int32) are device
 * pointers on the context's device; offset[] and n[] are HOST arrays, read
 * before the call returns.  Every in-range block's n*n elements at
 * d_dist + offset[b] must be readable device memory.  The staging buckets
 * are the context's, like the K1 workspace: a later ragged or K1 call on
 * another stream waits (hipStreamWaitEvent) for this call's last kernel. */
int tspgpu_solve_ragged_device(tspgpu_ctx *ctx, const void *d_dist, int dtype, const int64_t *offset,
                               const int32_t *n, int nblocks, void *d_cost, int32_t *d_tour, int tour_stride,
                               int32_t *d_status, void *hip_stream);
/* Host-pointer form, synchronous.  Uploads the covering extent
 * [min offset, max(offset + n*n)) of the in-range blocks in one copy — gaps
 * between blocks travel too, so this form is meant for packed (or nearly
 * packed) arrays — runs the device form on the context's stream and copies
 * cost, tour and status back. */
int tspgpu_solve_ragged(tspgpu_ctx *ctx, const void *dist, int dtype, const int64_t *offset, const int32_t *n,
                        int nblocks, void *cost_out, int32_t *tour_out, int tour_stride, int32_t *status_out);

/* ---------------------------------------------------------------------------
 * Distances on the device: the entry points above that start from cities
 * build the matrices on the host (glibc pow, two calls per entry) and upload
 * them.  These start from cities in device memory and leave the matrices
 * there, with the bits of tspgpu_distance_matrix: the device squares every
 * coordinate difference itself and lists the ~10% of squares that lie close
 * enough to a rounding midpoint for glibc's pow(x, 2) to differ from x*x; the
 * host runs pow on the listed operands only.  A non-finite
 * coordinate gives the NaN or infinite entries the host gives (a NaN's
 * payload aside), so such a block fails validation as it does there.
 *
 * d_cities: nblocks*n tspgpu_city (device).  Call-level errors (nothing is
 * launched): -EINVAL for a NULL context, a NULL pointer with nblocks > 0,
 * nblocks < 0 or n out of range; nblocks == 0 returns 0.  The fix-up list and
 * the matrices of the solve forms are the context's, grown on demand and
 * ordered against other work on the context like the K1 workspace.
 * ------------------------------------------------------------------------- */
/* computeDistanceMatrix into d_dist (nblocks*n*n doubles, device), n in
 * [1, TSPGPU_MAX_CITIES].  NOT fully asynchronous: the call synchronises
 * `hip_stream` once (after the build kernel, to run the host's pow; once more
 * in the rare case that the fix-up list overflowed and the build is repeated
 * with a larger one); the last two kernels are left running on the stream. */
int tspgpu_distance_matrix_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, int n, int nblocks, double *d_dist,
                                  void *hip_stream);
/* The matrices into a context buffer, then tspgpu_solve_ragged_device with
 * this n for every block: validation, d_status (nblocks int32), the NaN cost
 * and the row of -1 of a bad block are the ragged contract.  d_tour: rows of
 * n+1 entries.  n in [2, TSPGPU_MAX_CITIES] (strict: 16).  Synchronises the
 * stream as tspgpu_distance_matrix_device does; the solve is left running. */
int tspgpu_solve_cities_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, int n, int nblocks, double *d_cost,
                               int32_t *d_tour, int32_t *d_status, void *hip_stream);
/* tspgpu_solve_cities with the cities uploaded instead of the matrices;
 * synchronous, same outputs.  Return codes are tspgpu_solve_cities': the
 * first bad block's code (-EINVAL, -ERANGE) fails the call. */
int tspgpu_solve_cities_upload(tspgpu_ctx *ctx, const tspgpu_city *cities, int n, int nblocks, double *cost_out,
                               int32_t *tour_out);
/* The context's last device build, for tests and measurement: squares
 * computed (2 per unordered pair), squares sent to the host's pow, build
 * passes (2: the list overflowed once); and the host's wall time from the
 * first build launch to the end of its synchronisation (build kernel + the
 * copy of the list) and of the pow calls.  Any output pointer may be NULL. */
int tspgpu_cities_last_fixups(const tspgpu_ctx *ctx, uint64_t *squares, uint64_t *flagged, int *build_passes);
int tspgpu_cities_last_phase_ms(const tspgpu_ctx *ctx, double *build_ms, double *pow_ms);

/* ---------------------------------------------------------------------------
 * Ragged blocks from cities: blocks of DIFFERENT city counts,
 * PACKED.  Block b has n[b] cities at cities + (n[0] + ... + n[b-1]), in
 * caller order; n[] is a HOST array, read before the call returns.  The
 * packed layout is undefined unless every n[b] is in range, so an n[b]
 * outside [2, TSPGPU_MAX_CITIES] ([1, TSPGPU_MAX_CITIES] for the distance
 * form) is a call-level error: -EINVAL, nothing launched, no output written,
 * like a NULL context, a NULL pointer with nblocks > 0, nblocks < 0 or
 * tour_stride < (largest n[b]) + 1.  nblocks == 0 returns 0.  On a strict
 * context an n[b] of 17..20 is a per-block -EINVAL status instead (its cities
 * are skipped, the layout stays defined).
 * ------------------------------------------------------------------------- */
/* tspgpu_distance_matrix_device for packed ragged blocks: computeDistanceMatrix
 * of every block into d_dist, the matrices packed too (block b at element
 * n[0]^2 + ... + n[b-1]^2), each with the bits of tspgpu_distance_matrix on
 * that block alone.  Same protocol, fix-up list (a quarter of the sum of
 * n[b]*(n[b]-1) entries, or the knob DIST_FIX_CAP), overflow retry and
 * synchronisation as the uniform form; tspgpu_cities_last_fixups and
 * tspgpu_cities_last_phase_ms report this build too. */
int tspgpu_distance_matrix_ragged_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *n, int nblocks,
                                         double *d_dist, void *hip_stream);
/* The matrices into a context buffer, then tspgpu_solve_ragged_device with
 * the packed offsets: the ragged contract above applies unchanged (d_status,
 * NaN cost, a tour row of -1; rows of tour_stride entries, padded with -1).
 * A non-finite coordinate fails its own block only.  Synchronises the stream
 * as tspgpu_distance_matrix_device does; the solve is left running. */
int tspgpu_solve_cities_ragged_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *n, int nblocks,
                                      double *d_cost, int32_t *d_tour, int tour_stride, int32_t *d_status,
                                      void *hip_stream);
/* Host-pointer form, synchronous: uploads the cities, runs the device form on
 * the context's stream, copies cost, tour and status back.  Returns 0 however
 * many blocks are bad, like tspgpu_solve_ragged. */
int tspgpu_solve_cities_ragged(tspgpu_ctx *ctx, const tspgpu_city *cities, const int32_t *n, int nblocks,
                               double *cost_out, int32_t *tour_out, int tour_stride, int32_t *status_out);

/* Context-free convenience form (uses a per-thread default context on the
 * current device, created on first use). */
int tspgpu_solve(const double *dist, int n, int nblocks, double *cost_out, int32_t *tour_out,
                 const tspgpu_opts *opts);

/* Device memory, stream and timing helpers for callers that have no HIP
 * runtime of their own (ctypes / cgo / JNI users, bench.py): everything on the
 * context's device; copies are synchronous; the timer is a pair of HIP events
 * recorded on the context's stream (the stream the kernels run on when
 * hip_stream == tspgpu_stream(ctx)). */
int tspgpu_device_alloc(tspgpu_ctx *ctx, size_t bytes, void **ptr);
int tspgpu_device_free(tspgpu_ctx *ctx, void *ptr);
int tspgpu_memcpy_htod(tspgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
int tspgpu_memcpy_dtoh(tspgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
void *tspgpu_stream(tspgpu_ctx *ctx);
/* Extra non-blocking streams on the context's device (for callers without a
 * HIP runtime of their own), and a host wait on any stream. */
int tspgpu_stream_create(tspgpu_ctx *ctx, void **stream);
int tspgpu_stream_destroy(tspgpu_ctx *ctx, void *stream);
int tspgpu_stream_synchronize(tspgpu_ctx *ctx, void *stream);
int tspgpu_synchronize(tspgpu_ctx *ctx);
int tspgpu_timer_start(tspgpu_ctx *ctx);
int tspgpu_timer_stop(tspgpu_ctx *ctx, float *elapsed_ms);
/* CU count and device name of the context's device. */
int tspgpu_device_info(const tspgpu_ctx *ctx, int *cu_count, char *name, int namecap);

/* Device-side information for measurement: number of persistent workgroups
 * the last launch used and the DP relaxations per block for n cities,
 * N(N-1)2^(N-2) with N = n-1 (tsp.cpp:442-471). */
int tspgpu_last_grid(const tspgpu_ctx *ctx);
/* K1 variant the last batched launch used: 6 = sub-cube (hk_sub_kernel),
 * 4 = ping-pong + parent words, 2 = compact layer pass + prefetch (both
 * heldkarp_kernel); 0 for n = 2.  (1 and 5 named variants that were retired.) */
int tspgpu_last_variant(const tspgpu_ctx *ctx);
/* Measurement aid for variant 6, which runs two kernels per chunk of at
 * most 16384 blocks (the forward pass, then hk_tiled_backtrack): with split
 * timing enabled every chunk also records HIP events before, between and
 * after the two kernels, on the launch's stream.  tspgpu_k1_last_split_ms
 * waits for the last of them and returns both kernels' durations SUMMED over
 * every chunk of every launch since the previous read (or since enabling),
 * then starts a new sum: -ENOENT if nothing was recorded, -ENOSPC if more
 * than 4096 chunks were (recording stopped).  Enabling resets the sum. */
int tspgpu_k1_split_timing(tspgpu_ctx *ctx, int enable);
int tspgpu_k1_last_split_ms(tspgpu_ctx *ctx, float *forward_ms, float *backtrack_ms);
/* Number of visible HIP devices (0 when none). */
int tspgpu_device_count(void);
double tspgpu_relaxations_per_block(int n);
/* Algorithmic table bytes per block: every DP entry written once and read
 * once, 2 * 8 * N * 2^(N-1). */
double tspgpu_table_bytes_per_block(int n);

/* ---------------------------------------------------------------------------
 * K1-wide: ONE instance's Held-Karp with every CU of the GPU on each layer
 * (K1 gives each block one workgroup).  The single-instance time to the
 * optimal tour, and exact instances up to n = 31 (table N*2^(N-1) doubles:
 * 129 GB at n = 31).  Same cost and tour bits as K1 / tsp().  dist: n*n f64
 * (host); tour_out: n+1 entries; kernel_ms (optional): device time.
 * ------------------------------------------------------------------------- */
#define TSPGPU_WIDE_MAX_CITIES 31
int tspgpu_solve_instance(tspgpu_ctx *ctx, const double *dist, int n, double *cost_out, int32_t *tour_out,
                          double *kernel_ms);
/* K1-wide on int32 distances: the same DP, tie rule and tour layout; equals
 * tspgpu_solve_instance on the matrix converted to double.  n in [3, 31].
 * The table holds int32 values (half the bytes: 65 GB at n = 31), the
 * relaxation is an integer add and min.  -EINVAL: NULL pointer, n outside
 * [3, 31], any d < 0; -ERANGE: n * max(d) >= INT_MAX.  The context keeps one
 * workspace per (n, value type): an f64 call after an int32 call of the same
 * n, or the other way round, allocates anew. */
int tspgpu_solve_instance_i32(tspgpu_ctx *ctx, const int32_t *dist, int n, int32_t *cost_out,
                              int32_t *tour_out, double *kernel_ms);
/* value type of the context's last K1-wide launch: TSPGPU_F64, TSPGPU_I32, -1 if none
 * (set by both entries above and by K2's fallback; a measurement and test aid) */
int tspgpu_wide_last_dtype(const tspgpu_ctx *ctx);

/* ---------------------------------------------------------------------------
 * K2: exact search of ONE instance, prefix-parallel branch and bound over the
 * whole GPU (one instance per call instead of one block per workgroup), the
 * north_star's search shape for the reference's per-block problem
 * (tsp.cpp:405-509).  Same answer as tsp()/K1: the optimal left-fold cost and
 * the DP's tie-broken tour (see tspgpu_select_tour), for n <= 32 cities.
 * Distances: f64 (the reference's computeDistanceMatrix output) or i32 (the
 * integer-matrix extension: d >= 0, n * max(d) < 2^30).
 * ------------------------------------------------------------------------- */
#define TSPGPU_SEARCH_MAX_CITIES 32
/* (value types TSPGPU_F64 / TSPGPU_I32: defined above, with the ragged batches) */

/* One recorded complete tour: cost (IEEE bits of the f64 cost, or the
 * integer cost) and the inner cities t1..tN (N = n-1) in visiting order. */
typedef struct
{
    uint64_t cost;
    uint8_t city[32];
} tspgpu_tour_record;

typedef struct
{
    uint64_t nodes;         /* search nodes: child extensions cost + d[last][next] with their bound test */
    uint64_t records;       /* complete tours recorded at cost <= incumbent (last phase) */
    uint64_t optimal_tours; /* |O|: tours whose cost equals the optimum (0: not counted — the device tie
                               rule answered without the records being read, or K1-wide did) */
    uint64_t items;         /* prefixes (work items) N!/(N-D)! */
    int depth;              /* prefix depth D */
    int phases;             /* 1, or 2 when the record buffer overflowed (second search, bound = optimum) */
    int fallback;           /* 1: |O| too large to enumerate, the answer came from K1-wide (n <= 31) */
    int rounds;             /* search rounds of the last phase (items split and re-queued between rounds) */
    double kernel_ms;       /* device time of the search launches */
    uint64_t lane_steps;    /* lane slots of the search loop (64 per wave step) */
    uint64_t active_steps;  /* ... of which a lane worked on an item (lane utilisation = active/lane) */
    uint64_t item_loads;    /* items loaded by lanes (seeds and hand-backs) */
    int tie;                /* 1: the tour is the device tie rule's (tspgpu_tie_tour certified it) */
    int tie_checked;        /* 1: the records were also read and their host rule gave the same tour */
} tspgpu_search_stats;

/* Device tie rule (K2): the kernels keep, per recorded cost, the least
 * reverse-lexicographic key (t_N most significant) of the tours offered at
 * that cost; digit p = rank of t_(N-p) among the cities not placed yet, radix
 * N-p, in w0 for N <= 20, else digits 0..12 in w0 and the rest in w1.  This
 * decodes the key of the optimum's slot into tour_out (n+1 entries) and
 * certifies it as tsp()'s tour (tsp.cpp:457-470, 484-499): its fold must equal
 * cost_bits and, for f64, no fold one ulp below any of its prefixes may round
 * to the same next prefix (then every prefix fold is minimal and the DP's
 * backward argmin chain picks exactly this tour).  0: certified; -EAGAIN:
 * valid but not certified (use the records); -EINVAL: not a tour of that cost. */
int tspgpu_tie_tour(const void *dist, int dtype, int n, uint64_t w0, uint64_t w1, uint64_t cost_bits,
                    int32_t *tour_out);
/* The same certificate with the prefix DPs it may need run on the context's
 * GPU (K1-wide over the prefix's cities, up to 26; the host DP stops at 16),
 * so binade crossings late in long tours are proven too. */
int tspgpu_tie_tour_gpu(tspgpu_ctx *ctx, const void *dist, int dtype, int n, uint64_t w0, uint64_t w1,
                        uint64_t cost_bits, int32_t *tour_out);
/* tspgpu_tie_tour with the certificate's prefix minima taken from the
 * search's optimal records instead of a Held-Karp DP: records[0..count) must
 * be EVERY tour the search recorded (tspgpu_search_records with no overflow,
 * all shards), so that they hold the whole optimal set O; a prefix the records
 * cannot decide falls back to the DP on ctx's GPU (ctx may be NULL: then not
 * certified, -EAGAIN). */
int tspgpu_tie_tour_records(tspgpu_ctx *ctx, const void *dist, int dtype, int n, uint64_t w0, uint64_t w1,
                            uint64_t cost_bits, const tspgpu_tour_record *records, int count, int32_t *tour_out);
/* the key of a tour (tour[0] = 0, tour[1..n-1] = t1..tN): test helper */
int tspgpu_tie_key(int n, const int32_t *tour, uint64_t *w0, uint64_t *w1);

typedef struct tspgpu_search tspgpu_search; /* one instance (or one shard of it) on one context */

/* One-shot: whole instance on the context's GPU.  cost_out: the optimal cost
 * (an integer value for TSPGPU_I32); tour_out: n+1 entries 0,t1..tN,0.
 * When more tours tie for the optimum than can be enumerated (coincident
 * cities), n <= 31 is answered by K1-wide (stats->fallback = 1), larger n
 * return -EOVERFLOW. */
int tspgpu_search_solve(tspgpu_ctx *ctx, const void *dist, int dtype, int n, double *cost_out,
                        int32_t *tour_out, tspgpu_search_stats *stats);

/* Exhaustive enumeration (BASELINE config 2: "14-city exhaustive enumeration
 * on 1 MI355X"): the same search with the bound switched off — every one of
 * the (n-1)! tours is folded (the left fold of tsp.cpp), the tours within the
 * incumbent are recorded and the DP's tie rule picks among the optimal ones,
 * so the result equals tspgpu_search_solve / tsp().  stats->nodes counts every
 * partial path (about e*(n-1)!).  Practical up to ~16 cities on one GPU; this
 * one-shot is one shard on the context's GPU — to enumerate one instance over
 * several GPUs or ranks, create the shards with TSPGPU_SEARCH_EXHAUSTIVE
 * (below; bin/tsp_search --solver enum --gpus G, search_dist.solve_sharded). */
int tspgpu_search_enumerate(tspgpu_ctx *ctx, const void *dist, int dtype, int n, double *cost_out,
                            int32_t *tour_out, tspgpu_search_stats *stats);

/* Sharded form for multi-GPU drivers (one process or thread per GPU): shard s
 * of S seeds the depth-D prefixes p with p mod S == s (static interleave).
 * Inside the GPU the work runs in rounds: lanes take items from a device
 * queue, and an item that exceeds its iteration budget is split into the
 * untried siblings of each level of its stack, re-queued for the next round.
 * A driver calls start, then step until pending == 0, exchanging the
 * incumbent word between steps (e.g. RCCL all-reduce MIN of the u64 read with
 * tspgpu_search_counters, written back with tspgpu_search_set_bound); at the
 * end it all-reduces the incumbent, gathers the records whose cost equals it
 * from every shard and calls tspgpu_select_tour.  depth 0 = automatic. */
int tspgpu_search_create(tspgpu_ctx *ctx, const void *dist, int dtype, int n, int shard, int nshards, int depth,
                         tspgpu_search **out);
/* tspgpu_search_create with flags.  TSPGPU_SEARCH_DEVICE_BOUND: the create
 * launch also computes the initial incumbent on the device (nearest neighbour
 * from spread start cities + 2-opt, the cheaper left fold of either
 * direction; every shard of an instance gets the same bound), so a driver
 * needs no host heuristic and no tspgpu_search_set_bound before the search. */
#define TSPGPU_SEARCH_DEVICE_BOUND 1
/* TSPGPU_SEARCH_EXHAUSTIVE: this search is shard `shard` of `nshards` of the
 * exhaustive enumeration (tspgpu_search_enumerate's settings: no bound test,
 * the long round budget, knobs ENUM_KERNEL and SEARCH_RECORD_CAP).  Every
 * shard count gives the same bit-exact cost and tie-broken tour as tsp().
 *  - Shard rule.  For 7 <= n <= 16 the shard is ONE launch of the enumeration
 *    kernel: its work items are the (n-1)!/6! prefixes of depth n-7
 *    (tspgpu_search_info: depth, items), of which shard s folds p = i*S + s,
 *    i < local_items = items/S + (items % S > s) — the static interleave of
 *    the branch-and-bound seeds.  Other n (or knob ENUM_KERNEL=0) run the round
 *    kernels with the bound off over this shard's seeds.
 *  - Empty shards.  S may exceed the prefix count (n = 7 has one prefix, n = 8
 *    seven): a shard with local_items == 0 launches nothing, folds no tour,
 *    keeps its incumbent at the bound and reports no tie slot (found = 0).
 *  - The bound.  tspgpu_search_set_bound before the run, with the left-fold
 *    cost of a real tour, the same on every shard (tspgpu_heuristic_tour):
 *    tours within it are recorded, so a loose bound only costs records.
 *    TSPGPU_SEARCH_DEVICE_BOUND | TSPGPU_SEARCH_EXHAUSTIVE is not supported
 *    (-EINVAL).
 *  - tspgpu_search_run_all runs the shard (synchronous).  tspgpu_search_chain
 *    on an enumeration-kernel shard enqueues the one launch and the readbacks
 *    (counters, the shard's tie slot at its incumbent, first records) with one
 *    synchronisation, sets *done = 1 and calls the hook ZERO times: there are
 *    no levels, and no pruning an exchanged incumbent could help; the count
 *    is the same on every shard.  On the round kernels it returns *done = 0
 *    like any search that is not a chain: continue with start / step.
 *  - The winner over the shards is the branch-and-bound's: MIN of the
 *    incumbents, then MIN of the tie keys of the shards that hold a tour of
 *    that cost (tspgpu_search_tie_slot), else the records.
 *  - nodes (tspgpu_search_counters) counts every partial path: cumulative over
 *    the runs of a search (a second run_all with the optimum as the bound, the
 *    records fallback, adds its own), and the partial paths above the work
 *    items are counted by shard 0 alone, so the sum over the shards of one
 *    instance is exactly the one-shard count. */
#define TSPGPU_SEARCH_EXHAUSTIVE 2
int tspgpu_search_create_ex(tspgpu_ctx *ctx, const void *dist, int dtype, int n, int shard, int nshards, int depth,
                            int flags, tspgpu_search **out);
int tspgpu_search_destroy(tspgpu_search *s);
int tspgpu_search_info(const tspgpu_search *s, int *depth, uint64_t *items, uint64_t *local_items);
/* initial incumbent (a real tour's cost, e.g. tspgpu_heuristic_tour) */
int tspgpu_search_set_bound(tspgpu_search *s, double bound);
/* seed this shard's live prefixes (synchronous) */
int tspgpu_search_start(tspgpu_search *s);
/* one round over the pending items (synchronous); *pending = items left for the next round */
int tspgpu_search_step(tspgpu_search *s, uint64_t *pending);
/* start + steps until nothing is pending */
int tspgpu_search_run_all(tspgpu_search *s);
/* device time of all seed/round launches so far, and the rounds run */
int tspgpu_search_timing(const tspgpu_search *s, double *kernel_ms, int *rounds);
/* device address of the 64-bit incumbent word (f64 bits or integer cost).
 * The caller may write it (an RCCL all-reduce MIN in place): from this call
 * on tspgpu_search_counters / tspgpu_search_tie_slot read the device, not the
 * last chain's readback. */
void *tspgpu_search_incumbent_device(tspgpu_search *s);
int tspgpu_search_counters(tspgpu_search *s, uint64_t *incumbent_bits, uint64_t *nodes, uint64_t *records);
/* forget the records (and grow the buffer to `capacity` if larger) */
int tspgpu_search_reset_records(tspgpu_search *s, unsigned int capacity);
/* the recorded tours whose cost bits equal cost_bits; -EOVERFLOW if records
 * were lost (rerun with the optimum as the bound), -ENOSPC if cap is short */
int tspgpu_search_records(tspgpu_search *s, uint64_t cost_bits, tspgpu_tour_record *out, int cap, int *count);

/* Chained run of this shard (any shard count): the seeds,
 * every frontier level and the tail fold enqueued back to back on the
 * context's stream, ONE synchronisation, and the counters, this shard's tie
 * slot at its incumbent and its first records read back with it.  Between
 * levels, every `exchange_every` levels (0: never), hook(user, stream,
 * incumbent word) is called to enqueue an exchange of the device incumbent on
 * that stream — e.g. ncclAllReduce(word, word, 1, ncclUint64, ncclMin, comm,
 * stream): the same number of calls on every shard, chained or not.
 * *done = 1: the shard's search is complete.  *done = 0: the search is not
 * a chain — too large (a level overflowed, or n is above the chain's limit;
 * it is back at its starting state: incumbent restored, no records) or too
 * small to have a frontier level (below ~15 cities the seed depth, one prefix
 * per lane of the grid, already reaches the register tails: e.g. 13 cities,
 * seed depth 7 >= 12 - 6) — continue with tspgpu_search_start /
 * tspgpu_search_step.  The hooks are enqueued either way (same count). */
typedef void (*tspgpu_level_hook)(void *user, void *stream, void *incumbent_word);
int tspgpu_search_chain(tspgpu_search *s, int exchange_every, tspgpu_level_hook hook, void *user, int *done);

/* The device tie rule's least key among the tours this shard recorded at
 * cost cost_bits (tspgpu_tie_tour's w0/w1).  A driver of S shards takes the
 * all-reduce MIN of the incumbents (the optimum), then the MIN of w0 over the
 * shards (~0 where !found), then of w1 over the holders of that w0, and
 * certifies the winner once with tspgpu_tie_tour — the DP's tour without
 * gathering any record; overflow != 0 on any shard: the
 * records decide instead (tspgpu_search_records, tspgpu_select_tour). */
typedef struct
{
    uint64_t w0, w1; /* the key (w1 = 0 when n - 1 <= 20) */
    int found;       /* 1: a recorded tour of this shard has that cost */
    int overflow;    /* 1: the tie table lost an offer, the key may not be least */
} tspgpu_tie_slot;
int tspgpu_search_tie_slot(tspgpu_search *s, uint64_t cost_bits, tspgpu_tie_slot *out);

/* Host helpers.  A nearest-neighbour + 2-opt tour and its left-fold cost (an
 * upper bound); and the DP's tie rule applied to the optimal set O: walking
 * from the last city backwards, take the smallest m that ends a tour of O with
 * the chosen suffix and whose best prefix fold + d[m][next] equals the state
 * value (tsp.cpp:457-470, 483-499) — the tour tsp() returns. */
int tspgpu_heuristic_tour(const void *dist, int dtype, int n, double *cost_out, int32_t *tour_out);
/* the same over the start cities first, first + step, ... < n only (-ENOENT
 * when first >= n): R ranks taking first = r, step = R and the MIN of their
 * costs get the bound of all starts, each doing 1/R of the work */
int tspgpu_heuristic_tour_starts(const void *dist, int dtype, int n, int first, int step, double *cost_out,
                                 int32_t *tour_out);
int tspgpu_select_tour(const void *dist, int dtype, int n, const tspgpu_tour_record *records, int count,
                       uint64_t cost_bits, int32_t *tour_out);

/* ---------------------------------------------------------------------------
 * K3: the reference's mergeBlocks (tsp.cpp:197-269) and its reduction tree
 * (MPI_ManualReduce tsp.cpp:52-134 + the local fold tsp.cpp:348-352) with the
 * paths on the GPU.  Same result as the reference bit for bit: the L1 x L2
 * swap search runs on the device, near-minimal candidates are re-evaluated
 * on the host with glibc pow (assignment2.h:141-144), the splice is a device
 * gather.  Cities are the reference's City structs, paths include the
 * closing city like BlockSolution.path.
 * ------------------------------------------------------------------------- */
/* mergeBlocks(p1, p2): out (L1+L2-1 cities), *cost_out = c1 + c2 + best swap.
 * Returns the merged length, or a negative code. */
int tspgpu_merge(tspgpu_ctx *ctx, const tspgpu_city *p1, int L1, double c1, const tspgpu_city *p2, int L2, double c2,
                 tspgpu_city *out, double *cost_out);
/* The distribution counts, every logical rank's left fold and the reduction
 * tree for logical rank count nprocs, given each block's solution (paths of
 * L cities, block-major).  Writes the final cost and the "process %i is about
 * to receive %i cities from process %i" lines (tsp.cpp:88) into log. */
int tspgpu_reduce(tspgpu_ctx *ctx, const tspgpu_city *paths, int L, const double *costs, int nblocks, int nprocs,
                  double *final_cost, char *log, int logcap);
/* tspgpu_reduce, and the merged tour: rank 0's final path (cities, closing
 * city included; with nprocs > 1 the reference's stale receive lists can
 * repeat cities, so the length is data-dependent).  *path_len is always set
 * to the full length; path_out receives min(len, path_cap) cities; a short
 * path_cap returns -ENOSPC after final_cost, log and *path_len are written.
 * path_out may be NULL with path_cap 0 (length query).  -EINVAL also for a
 * NULL path_len, path_cap < 0, or a NULL path_out with path_cap > 0. */
int tspgpu_reduce_path(tspgpu_ctx *ctx, const tspgpu_city *paths, int L, const double *costs, int nblocks,
                       int nprocs, double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len, char *log,
                       int logcap);
/* The same from K1's device outputs, without a visit to the host: d_cities
 * (nblocks*n), d_tour (rows of n+1), d_cost (nblocks doubles), d_status
 * (nblocks int32, or NULL: the caller guarantees every block is valid) are
 * device pointers on the context's device, produced on hip_stream; the
 * reduce runs on the context's stream after an event wait on hip_stream.
 * d_path_out: device, path_cap cities (may be NULL with path_cap 0).
 * Synchronous (the merge needs host decisions).  One device pass gathers the
 * block paths (convPathToCityPath, assignment2.h:76-84) and takes the facts
 * tspgpu_reduce scans its host paths for — exact coordinate extrema, so the
 * candidate window is bit-equal to tspgpu_reduce's — and only the nblocks
 * costs come to the host (the cost fold stays there, in merge order, with
 * glibc).  A non-zero status fails the call with the first such block's code
 * before anything is merged (d_path_out untouched; such a block's tour row
 * is never read); a tour entry outside [0, n) under status 0 -> -EINVAL
 * (checked before it indexes anything); non-finite coordinates -> -EINVAL;
 * -EDEADLK as tspgpu_reduce.  n in [2, TSPGPU_MAX_CITIES], nblocks * (n+1)
 * <= INT_MAX.  Same cost, log and path as tspgpu_reduce_path on the gathered
 * paths for any input; ids spread wider than 8 * nblocks * (n+1) are not
 * checked for uniqueness on the device and take the general per-merge path
 * where the host form may take the one-kernel folds (same answer, slower). */
int tspgpu_reduce_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *d_tour, const double *d_cost,
                         const int32_t *d_status, int n, int nblocks, int nprocs, double *final_cost,
                         tspgpu_city *d_path_out, int path_cap, int *path_len, char *log, int logcap,
                         void *hip_stream);
/* Device time of the context's last tspgpu_reduce_device's gather, summary
 * and uniqueness kernels (HIP events); a measurement aid. */
int tspgpu_reduce_device_last_ms(const tspgpu_ctx *ctx, double *gather_ms);
/* Cities on the host in, final cost / merged tour / log out: uploads the
 * cities, tspgpu_solve_cities_device, tspgpu_reduce_device, one copy of the
 * path back.  Buffers are per call.  Return codes: tspgpu_solve_cities_upload's
 * for the block search (the first bad block's code), tspgpu_reduce_path's for
 * the merge. */
int tspgpu_pipeline_cities(tspgpu_ctx *ctx, const tspgpu_city *cities, int n, int nblocks, int nprocs,
                           double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len, char *log,
                           int logcap);
/* The three forms above for blocks of DIFFERENT sizes (the
 * reference's mergeBlocks takes two paths of any length).  Call-level errors
 * as above, and -EINVAL for nblocks < 1, a NULL n / len, or any n[b] outside
 * [2, TSPGPU_MAX_CITIES] (len[b] < 2): nothing is launched or written. */
/* tspgpu_reduce_device for the outputs of tspgpu_solve_cities_ragged_device:
 * packed cities (n[] a HOST array), tour rows of tour_stride >= (largest
 * n[b]) + 1 entries; block b's path is tspgpu_tour_length(n[b]) cities.
 * Status, tour entry (outside [0, n[b])), non-finite, -EDEADLK and -ENOSPC
 * behave as there; the sum of the path lengths must be <= INT_MAX.  Ids
 * spread wider than 8 * (that sum) take the general per-merge path, as does
 * any batch with a 2-city block (an open path). */
int tspgpu_reduce_ragged_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, const int32_t *n, const int32_t *d_tour,
                                int tour_stride, const double *d_cost, const int32_t *d_status, int nblocks,
                                int nprocs, double *final_cost, tspgpu_city *d_path_out, int path_cap, int *path_len,
                                char *log, int logcap, void *hip_stream);
/* tspgpu_reduce_path for paths of different lengths, for block tours from
 * anywhere: paths is the concatenation, path b has len[b] >= 2 cities (host
 * arrays).  tspgpu_reduce_path's contract; paths longer than 33 cities take
 * the per-merge kernels instead of the one-kernel fold (same answer). */
int tspgpu_reduce_ragged(tspgpu_ctx *ctx, const tspgpu_city *paths, const int32_t *len, const double *costs,
                         int nblocks, int nprocs, double *final_cost, tspgpu_city *path_out, int path_cap,
                         int *path_len, char *log, int logcap);
/* tspgpu_pipeline_cities for packed ragged blocks: upload,
 * tspgpu_solve_cities_ragged_device, tspgpu_reduce_ragged_device, one copy of
 * the tour back.  Return codes are tspgpu_pipeline_cities'. */
int tspgpu_pipeline_cities_ragged(tspgpu_ctx *ctx, const tspgpu_city *cities, const int32_t *n, int nblocks,
                                  int nprocs, double *final_cost, tspgpu_city *path_out, int path_cap, int *path_len,
                                  char *log, int logcap);

/* ---------------------------------------------------------------------------
 * Fixed-end shortest paths and the window refinement of a tour (DESIGN.md
 * §6d; an extension: the reference has no counterpart).
 *
 * A path problem is a block of w cities, or a w x w row-major matrix D, with
 * 4 <= w <= TSPGPU_MAX_CITIES (strict: 17).  Local city 0 is the fixed start,
 * city w-1 the fixed end, the m = w-2 interior cities may be reordered.  The
 * answer is the order 0, t1..tm, w-1 whose left fold
 * ((D[0][t1] + D[t1][t2]) + ...) + D[tm][w-1] is minimal, DEFINED as what
 * tspgpu_solve_blocks returns for the w-1 cities of the folded matrix P:
 *   P[i][j] = D[i][j] for j >= 1,  P[i][0] = D[i][w-1] for i >= 1,  P[0][0] = 0
 * cost bit for bit, the order K1's tour with its closing 0 replaced by w-1 (so
 * ties break as K1 breaks them on P).  Only D[0][1..w-2], D[i][j] with i, j in
 * 1..w-2 and D[1..w-2][w-1] are read: row w-1 and column 0 never are.
 * Validation, status[b] and a bad block's outputs (cost NaN / -1, an order row
 * of -1, neighbours solved) are the ragged contract above applied to P.
 *
 * Call-level errors (nothing launched, nothing written): -EINVAL for a NULL
 * context, w outside [4, 20] (strict: 17), nblocks < 0, an unknown dtype, a
 * NULL pointer with nblocks > 0.  nblocks == 0 returns 0.  Order rows have w
 * entries.
 * ------------------------------------------------------------------------- */
/* Device-pointer form, asynchronous on `hip_stream` like
 * tspgpu_solve_ragged_device.  d_dist: nblocks*w*w elements of dtype
 * (TSPGPU_F64 / TSPGPU_I32), d_cost: nblocks of them, d_order: nblocks*w
 * int32, d_status: nblocks int32. */
int tspgpu_solve_paths_device(tspgpu_ctx *ctx, const void *d_dist, int dtype, int w, int nblocks, void *d_cost,
                              int32_t *d_order, int32_t *d_status, void *hip_stream);
/* Host-pointer form, synchronous.  Returns 0 however many blocks are bad. */
int tspgpu_solve_paths(tspgpu_ctx *ctx, const void *dist, int dtype, int w, int nblocks, void *cost_out,
                       int32_t *order_out, int32_t *status_out);
/* From cities (nblocks*w tspgpu_city): the matrices come from the exact device
 * build (the bits of tspgpu_distance_matrix), which synchronises the stream as
 * tspgpu_distance_matrix_device does; the solve is left running. */
int tspgpu_solve_paths_cities_device(tspgpu_ctx *ctx, const tspgpu_city *d_cities, int w, int nblocks,
                                     double *d_cost, int32_t *d_order, int32_t *d_status, void *hip_stream);
int tspgpu_solve_paths_cities(tspgpu_ctx *ctx, const tspgpu_city *cities, int w, int nblocks, double *cost_out,
                              int32_t *order_out, int32_t *status_out);

/* Window refinement.  A path is L >= 2 cities like BlockSolution.path; its two
 * end cities never move (they need not be equal).  m, 2 <= m <= 18 (strict:
 * 15), is the interior count of a window.  Pass p = 0, 1, ... uses the offset
 * o_p = 0 (p even) or (m+1)/2 (p odd); its window k starts at position
 * s = o_p + k(m+1) and covers s .. s+m+1, both ends fixed and shared with the
 * neighbours, k < W_p = max(0, (L-1-o_p) / (m+1)).  Positions no window covers
 * stay.  Every window is one path problem on tspgpu_distance_matrix of its
 * m+2 cities; its old cost is the left fold of the identity order on that
 * matrix; its interior is replaced by the solved order iff status == 0 and
 * new < old strictly (a tie keeps the old order); gain_k = old - new for a
 * replaced window, else 0.  The loop ends after pass p when p+1 == max_passes,
 * or when p >= 1 and neither pass p nor pass p-1 replaced a window (an empty
 * pass replaces none).  The result is a permutation of the input with both
 * ends in place, and deterministic.  A path too short for any window
 * (L < m+2) returns 0 with zero stats and the path untouched.
 * -EINVAL: NULL context or path, L < 2, m out of range, max_passes < 1. */
typedef struct
{
    int passes;           /* passes run (empty ones included) */
    int64_t windows;      /* windows solved */
    int64_t replaced;     /* windows whose interior was replaced */
    int64_t skipped;      /* windows of status != 0 (left as they were) */
    double gain;          /* left fold of gain_k on the host, in pass order then window order */
    /* a measurement aid: device time (HIP events) summed over the passes of
     * gather + distance build (the host's pow included), of K1 (with its
     * validation gather and scatter) and of fold + apply */
    double build_ms, k1_ms, fold_apply_ms;
} tspgpu_refine_stats;
/* In place on the device; synchronous (the host decides after every pass
 * whether to stop, as tspgpu_reduce_device's merges need host decisions).
 * stats may be NULL. */
int tspgpu_refine_path_device(tspgpu_ctx *ctx, tspgpu_city *d_path, int L, int m, int max_passes,
                              tspgpu_refine_stats *stats, void *hip_stream);
/* Host form: path up, the device form on the context's stream, path_out (L
 * cities; may be path itself) down. */
int tspgpu_refine_path(tspgpu_ctx *ctx, const tspgpu_city *path, int L, int m, int max_passes, tspgpu_city *path_out,
                       tspgpu_refine_stats *stats);
/* The yardstick for before and after, on the host with glibc: the left fold,
 * in path order, of the reference's distance() (assignment2.h:141-144) on
 * consecutive cities.  L >= 1 (one city: 0). */
int tspgpu_path_length(const tspgpu_city *path, int L, double *len);

/* ---------------------------------------------------------------------------
 * 2-opt with a neighbour grid (an extension: the reference has
 * no counterpart).  The stage in front of the window refinement: it repairs
 * what no window can hold, two edges close in the plane and far apart in tour
 * order.  The whole contract is below; tests/two_opt_model.py is the same in
 * Python, and the device matches it bit for bit.
 *
 * A path is L cities like BlockSolution.path, 1 <= L <= 2^30.  Positions 0
 * and L-1 never move and need not be equal.  "City" means the index a city
 * had in the input; coincident and duplicate cities are ordinary cities.
 *
 * Distance.  d(a,b) = sqrt(dx*dx + dy*dy), dx = a.x - b.x, dy = a.y - b.y, in
 * f64, every operation rounded on its own (no contraction), sqrt correctly
 * rounded.  It is the search's metric, not the reference's pow form:
 * tspgpu_path_length stays the yardstick for before and after.
 *
 * Validation, before anything is written.  -EINVAL: a NULL context or path,
 * L < 1 (or above 2^30), ring outside 1..4, max_passes < 1, any non-finite
 * coordinate.  -ERANGE: with ex = xmax - xmin and ey = ymax - ymin over all L
 * cities, ex, ey or ex*ex + ey*ey not finite.  L < 4 (after these checks): 0
 * with passes = 0 and the path untouched.  On an error neither the path nor
 * *stats is written.
 *
 * Grid, built once per call (cities do not move, only their positions).  g
 * is the largest integer with 2*g*g <= L, clamped to [1, 2048].  The cell of
 * a city is cx = min(g-1, (int)(((x - xmin) / ex) * g)), 0 when ex == 0, and
 * cy likewise on y: an IEEE division, then the product.  N(c) is every city,
 * c included, whose cell is within `ring` cells of c's in both coordinates,
 * clipped at the border; N is symmetric.
 *
 * Moves.  With p the current order, move (i, j) is defined for 0 <= i,
 * i+2 <= j <= L-2.  With a = p[i], b = p[i+1], c = p[j], e = p[j+1],
 *   gain = (d(a,b) + d(c,e)) - (d(a,c) + d(b,e))
 * in exactly that order of operations, and applying it reverses positions
 * i+1..j.  The candidates of position i are the j with c in N(a) or e in
 * N(b); a j found both ways is one candidate.  The best move of i is the
 * largest gain among its candidates with gain > 0, the smallest j on equal
 * gains; it may not exist.  Nothing prunes the candidates.
 *
 * A pass.  (1) The best move of every i, all under the order at the start of
 * the pass.  (2) Sort the existing ones by (gain descending, i ascending).
 * (3) In that order accept a move iff its edge range [i, j] is disjoint from
 * that of every move accepted before: (i, j) and (j+1, j') are compatible,
 * sharing edge j is not.  (4) gain = gain + g_k for every accepted move in
 * acceptance order, a left fold.  (5) Apply all accepted reversals.  A pass
 * that accepts nothing is counted and ends the call, as does reaching
 * max_passes.  Every choice is a total order, so the result is a function of
 * the input alone: a permutation of it with both ends in place.
 * ------------------------------------------------------------------------- */
typedef struct
{
    int passes;         /* passes run (the last, empty one included) */
    int64_t candidates; /* best moves sent to the selection, summed over the passes */
    int64_t moves;      /* moves accepted and applied */
    double gain;        /* the left fold of the accepted gains */
    /* a measurement aid: device time (HIP events) of bounds + grid build, of
     * the searches and of the applies, and the host's time in the selection,
     * each summed over the passes */
    double grid_ms, search_ms, select_ms, apply_ms;
} tspgpu_two_opt_stats;
/* In place on the device; synchronous (the host selects after every pass).
 * stats may be NULL. */
int tspgpu_two_opt_path_device(tspgpu_ctx *ctx, tspgpu_city *d_path, int L, int ring, int max_passes,
                               tspgpu_two_opt_stats *stats, void *hip_stream);
/* Host form: path up, the device form on the context's stream, path_out (L
 * cities; may be path itself) down. */
int tspgpu_two_opt_path(tspgpu_ctx *ctx, const tspgpu_city *path, int L, int ring, int max_passes,
                        tspgpu_city *path_out, tspgpu_two_opt_stats *stats);

/* ---------------------------------------------------------------------------
 * Or-opt with a neighbour grid (an extension: the reference
 * has no counterpart).  Segment insertion, the move that neither 2-opt nor a
 * window reaches: 1 to 3 consecutive cities leave the tour and go back in,
 * either way round, next to a city that is close in the plane and arbitrarily
 * far in tour order.  The whole contract is below and in "2-opt with a
 * neighbour grid" above; tests/or_opt_model.py is the same in Python, and the
 * device matches it bit for bit.
 *
 * Unchanged from 2-opt: a path of 1 <= L <= 2^30 cities, "city" = index in
 * the input; the distance d (f64, no contraction, correctly rounded sqrt);
 * the validation, its codes and their order, with nothing written on an
 * error; the grid, g, the cell formula and N(c) with ring in 1..4; positions
 * 0 and L-1 never move.  New: max_seg outside 1..3 is -EINVAL with the other
 * arguments.  L < 4 (after the checks): 0 with passes = 0, the path untouched.
 *
 * Moves.  With p the current order, move (a, k, t, rev) takes the segment of
 * positions a..h, h = a+k-1, 1 <= k <= max_seg, 1 <= a, h <= L-2, and puts it
 * into edge t (between positions t and t+1), 0 <= t <= L-2, t outside
 * [a-1, h].  With first = p[a], last = p[h], P = p[a-1], N = p[h+1], c = p[t],
 * e = p[t+1]: rev = 0 puts the segment in as it lies, x = first follows c and
 * y = last precedes e; rev = 1 puts it in reversed, x = last and y = first;
 * k = 1 has rev = 0 only.
 *   gain = ((d(P,first) + d(last,N)) + d(c,e)) - ((d(P,N) + d(c,x)) + d(y,e))
 * in exactly that order of operations: a function of the move, not of how it
 * was found.  Applying it: if t > h, positions a..t become p[h+1..t] followed
 * by the (reversed) segment, and its edge range is [lo, hi] = [a-1, t]; if
 * t < a-1, positions t+1..h become the (reversed) segment followed by
 * p[t+1..a-1], and [lo, hi] = [t, h].  Either way a rotation of positions
 * lo+1..hi.
 *
 * Candidates of position s, 1 <= s <= L-2, f = p[s]: the segments with f at
 * one end, [s, s+k-1] and [s-k+1, s] for k <= max_seg, those that leave
 * 1..L-2 dropped, k = 1 counted once; for each of them and every v in N(f),
 * v != f, at position q, the two insertions that make f adjacent to v:
 * t = q (c = v, f is x) and t = q-1 (e = v, f is y), rev following from the
 * end f is and the side it lands on; illegal t dropped.  The best move of s
 * is the largest gain > 0, on equal gains the lexicographically smallest
 * (a, k, t, rev); a move reached twice is one move; it may not exist.
 * Nothing prunes the candidates.  A segment whose other end is the one near v
 * is found by that end's position, so the neighbourhood is complete, and one
 * move may be reported by two positions.
 *
 * A pass.  (1) The best move of every s, all under the order at the start of
 * the pass.  (2) Sort the existing ones by (gain descending, s ascending).
 * (3) In that order accept a move iff its [lo, hi] is disjoint from that of
 * every move accepted before; hi + 1 = lo' is compatible.  (4) gain = gain +
 * g_k for every accepted move in acceptance order, a left fold.  (5) Apply
 * all accepted moves.  A pass that accepts nothing is counted and ends the
 * call, as does reaching max_passes.  Every choice is a total order, so the
 * result is a function of the input alone: a permutation of it with both
 * ends in place.
 * ------------------------------------------------------------------------- */
typedef struct
{
    int passes;         /* passes run (the last, empty one included) */
    int64_t candidates; /* best moves sent to the selection, summed over the passes */
    int64_t moves;      /* moves accepted and applied */
    double gain;        /* the left fold of the accepted gains */
    /* as in tspgpu_two_opt_stats (apply_ms: the stage and commit kernels) */
    double grid_ms, search_ms, select_ms, apply_ms;
} tspgpu_or_opt_stats;
/* In place on the device; synchronous (the host selects after every pass).
 * stats may be NULL. */
int tspgpu_or_opt_path_device(tspgpu_ctx *ctx, tspgpu_city *d_path, int L, int ring, int max_seg, int max_passes,
                              tspgpu_or_opt_stats *stats, void *hip_stream);
/* Host form: path up, the device form on the context's stream, path_out (L
 * cities; may be path itself) down. */
int tspgpu_or_opt_path(tspgpu_ctx *ctx, const tspgpu_city *path, int L, int ring, int max_seg, int max_passes,
                       tspgpu_city *path_out, tspgpu_or_opt_stats *stats);

/* ---------------------------------------------------------------------------
 * Tuning and test knobs.  The defaults are the measured best; a knob changes
 * how the kernels run (K1 variant / configuration, buffer sizes, a bound
 * switched off for an A/B run, a fallback forced by a test), never the
 * answer.  Process-wide, read where each is used (K1 knobs at context
 * creation, K2 knobs at search creation).  The library reads no environment
 * variable of its own: the documented TSP_* variables belong to bin/tsp.
 * Names: K1, TILED_CFG, K1_CHUNK, WG_PER_CU, THREADS, LDS_TABLE_MAX_N, WIDE_PULL,
 * SEARCH_{KERNEL, HUNGRY, MIN_SPLIT, WALL_S, RING_LOG2, REFILL, TAIL, SUFFIX,
 * TWO_EDGE, CHAIN, LAGRANGE, MST, MST_MINREM, TAIL_CAP_LOG2, EXPAND_LOG2,
 * BUDGET, TIE, PAGEABLE, TAILS, CHAIN_CAP_LOG2, CHAIN_POISON, DEBUG, DEPTH,
 * RECORD_CAP}, CHAIN_FPB, CHAIN_GRID, ENUM_KERNEL, ENUM_WG_PER_CU,
 * HEURISTIC_THREADS, HEURISTIC_ALL_STARTS, DIST_FIX_CAP (csrc/tuning.cpp).
 * ------------------------------------------------------------------------- */
/* 0, -ENOENT (no such knob) or -EINVAL (not finite) */
int tspgpu_tuning_set(const char *name, double value);
/* back to the default (name NULL: every knob) */
int tspgpu_tuning_clear(const char *name);

#ifdef __cplusplus
}
#endif
#endif
