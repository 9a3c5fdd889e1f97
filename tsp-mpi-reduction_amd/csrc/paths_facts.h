// The facts of the K1 -> K3 hand-off (paths.h) and the rules
// the host applies to them, one copy for the kernels (paths.hip), the front
// (merge.hip) and the host check (host/check_paths.cpp).
//
// Every unit that includes this is built with -ffp-contract=off: the diagonal
// must round where it is written, as in the host scan.
#pragma once
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TSPGPU_PATHS_HD __host__ __device__ inline
#else
#define TSPGPU_PATHS_HD inline
#endif

namespace tspgpu {

enum : unsigned {
    kPathNonFinite = 1u,  // a gathered coordinate is NaN or infinite
    kPathBadIndex = 2u,   // a tour entry outside [0, n) under status 0
    kPathOpen = 4u,       // a path's last city's id differs from its first city's
    kPathDupId = 8u,      // an id occurs twice (closing copies aside)
    kPathWideIds = 16u,   // id_max - id_min >= 8*B*L: uniqueness not decided
};

// The device words of one hand-off (the host uploads path_facts_init()).
struct PathFacts {
    unsigned long long xmin, xmax, ymin, ymax;  // path_order_key of the extrema
    unsigned long long first_bad;  // (block << 32) | (uint32) status of the first non-zero status; ~0: none
    int id_min, id_max;
    unsigned flags;
    unsigned pad;
};

inline PathFacts path_facts_init()
{
    PathFacts f{};
    f.xmin = f.ymin = ~0ull;
    f.xmax = f.ymax = 0ull;
    f.first_bad = ~0ull;
    f.id_min = INT_MAX;
    f.id_max = INT_MIN;
    return f;
}

// Monotone map of the finite doubles (and the infinities) onto unsigned
// integers: a < b  =>  key(a) < key(b); -0.0 sorts below +0.0, which no
// caller can see (an extremum only enters a difference that is squared).
// No finite value's key is 0 or ~0: both serve as "nothing seen".
TSPGPU_PATHS_HD unsigned long long path_order_key(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
TSPGPU_PATHS_HD double path_key_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __builtin_bit_cast(double, b);
}

// bits (= bytes * 8) of the uniqueness bitmap of nblocks paths of L cities
TSPGPU_PATHS_HD unsigned long long path_bitmap_bits(int nblocks, int L)
{
    return 8ull * (unsigned long long)nblocks * (unsigned long long)L;
}
// its allocation: whole 32-bit words (the kernel addresses it with atomicOr on
// words, and nblocks * L need not be a multiple of 4)
TSPGPU_PATHS_HD unsigned long long path_bitmap_bytes(int nblocks, int L)
{
    return (path_bitmap_bits(nblocks, L) + 31ull) / 32ull * 4ull;
}
// the bitmap rule: the ids [id_min, id_max] fit the bitmap
TSPGPU_PATHS_HD bool path_ids_fit_bitmap(long long id_min, long long id_max, int nblocks, int L)
{
    return id_max >= id_min && (unsigned long long)(id_max - id_min) < path_bitmap_bits(nblocks, L);
}

// The same three for paths of different lengths, over the
// total count of gathered cities (closing copies included): for nblocks paths
// of L cities each, total = nblocks * L gives the values above.
TSPGPU_PATHS_HD unsigned long long path_bitmap_bits_total(unsigned long long total) { return 8ull * total; }
TSPGPU_PATHS_HD unsigned long long path_bitmap_bytes_total(unsigned long long total)
{
    return (path_bitmap_bits_total(total) + 31ull) / 32ull * 4ull;
}
TSPGPU_PATHS_HD bool path_ids_fit_bitmap_total(long long id_min, long long id_max, unsigned long long total)
{
    return id_max >= id_min && (unsigned long long)(id_max - id_min) < path_bitmap_bits_total(total);
}

// The diagonal of the bounding box [x0, x1] x [y0, y1], padded: Dmax of K3's
// candidate window (merge.hip).  One formula for the host scan of
// tspgpu_reduce and for the extrema the device summary brings, so both give
// the same bits.
inline double path_bbox_diagonal(double x0, double x1, double y0, double y1)
{
    if (!(x1 >= x0) || !(y1 >= y0)) return 0.0;
    return sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0)) * (1.0 + 1e-9) + 1e-300;
}
inline double path_facts_diagonal(const PathFacts &f)
{
    if (f.xmin == ~0ull || f.ymin == ~0ull) return 0.0;  // (nothing gathered)
    return path_bbox_diagonal(path_key_value(f.xmin), path_key_value(f.xmax), path_key_value(f.ymin),
                              path_key_value(f.ymax));
}

// What fails the call before anything is merged: the first block with a
// non-zero status (its code), then a bad index or a non-finite coordinate.
inline int path_facts_error(const PathFacts &f)
{
    if (f.first_bad != ~0ull) {
        const int code = (int)(uint32_t)(f.first_bad & 0xffffffffull);
        return code < 0 ? code : -EIO;  // (statuses are negative errno values)
    }
    return (f.flags & (kPathBadIndex | kPathNonFinite)) ? -EINVAL : 0;
}

// the one-kernel fold merges' precondition: paths of at least 3 cities that
// close on their first city, ids proven unique across blocks
inline bool path_facts_fold_ok(const PathFacts &f, int L)
{
    return L >= 3 && !(f.flags & (kPathOpen | kPathDupId | kPathWideIds));
}
// the same for paths of different lengths: EVERY path has at least 3 cities
// (min_len: the shortest path's length)
inline bool path_facts_fold_ok_ragged(const PathFacts &f, int min_len) { return path_facts_fold_ok(f, min_len); }

}  // namespace tspgpu
