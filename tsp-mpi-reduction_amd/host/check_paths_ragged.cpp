// host/check_paths.cpp for blocks of DIFFERENT sizes, without
// a GPU: a serial twin of the ragged summary and bitmap (paths.hip's
// paths_gather_ragged_kernel and paths_unique_ragged_kernel over the
// descriptor table of block_desc.h: packed cities, tour rows of one stride,
// concatenated paths, the total-count bitmap rule of paths_facts.h) against
// the ragged host scan of tspgpu_reduce_ragged (finite, bounding box, "every
// path has at least 3 cities and closes", a sort of every id).  Random ragged
// batches with every id layout of check_paths.cpp (the widest range that
// still fits, ending on the bitmap's last bit with a total that is no
// multiple of 4, included), 2-city blocks mixed in, statuses, bad indices and
// non-finite coordinates; no index leaves its array (the program runs under
// ASan + UBSan too: `make check-paths-ragged`).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "block_desc.h"
#include "paths_facts.h"
#include "tspgpu.h"

using namespace tspgpu;

namespace {

int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            ++fails;                                                  \
        }                                                             \
    } while (0)

int tour_len(int n) { return n == 2 ? 2 : n + 1; }

// the table the fronts build from n[]
std::vector<BlockDesc> table_of(const std::vector<int32_t> &n)
{
    std::vector<BlockDesc> t(n.size());
    int64_t city = 0, dist = 0, path = 0;
    for (size_t b = 0; b < n.size(); ++b) {
        t[b] = BlockDesc{city, dist, path, n[b], tour_len(n[b])};
        city += n[b], dist += (int64_t)n[b] * n[b], path += tour_len(n[b]);
    }
    return t;
}

// what the two ragged kernels compute, serially
PathFacts twin(const std::vector<tspgpu_city> &cities, const std::vector<int32_t> &tour, int stride,
               const int32_t *status, const std::vector<BlockDesc> &desc, std::vector<tspgpu_city> &paths)
{
    const int B = (int)desc.size();
    size_t total = 0;
    int min_len = INT_MAX;
    for (const BlockDesc &e : desc) total += (size_t)e.L, min_len = std::min(min_len, (int)e.L);
    PathFacts f = path_facts_init();
    paths.assign(total, tspgpu_city{-12345, -1.0, -1.0});
    for (int b = 0; b < B; ++b) {
        const BlockDesc &e = desc[b];
        if (status && status[b] != 0) {
            const unsigned long long w = ((unsigned long long)b << 32) | (unsigned)status[b];
            f.first_bad = std::min(f.first_bad, w);
            continue;  // the row is never read
        }
        bool rowbad = false;
        for (int i = 0; i < e.L; ++i) {
            const int t = tour.at((size_t)b * stride + i);
            if (t < 0 || t >= e.n) rowbad = true;
        }
        if (rowbad) {
            f.flags |= kPathBadIndex;
            continue;
        }
        for (int i = 0; i < e.L; ++i) {
            const tspgpu_city c = cities.at((size_t)e.city + tour[(size_t)b * stride + i]);
            paths.at((size_t)e.path + i) = c;
            f.id_min = std::min(f.id_min, c.id);
            f.id_max = std::max(f.id_max, c.id);
            for (int k = 0; k < 2; ++k) {
                const double v = k ? c.y : c.x;
                unsigned long long &lo = k ? f.ymin : f.xmin, &hi = k ? f.ymax : f.xmax;
                if (!std::isfinite(v)) {
                    f.flags |= kPathNonFinite;
                } else {
                    lo = std::min(lo, path_order_key(v));
                    hi = std::max(hi, path_order_key(v));
                }
            }
        }
        if (paths[(size_t)e.path + e.L - 1].id != paths[(size_t)e.path].id) f.flags |= kPathOpen;
    }
    // (the front allocates no bitmap when some path has fewer than 3 cities)
    if (min_len < 3 || f.first_bad != ~0ull || (f.flags & kPathBadIndex)) return f;
    if (!path_ids_fit_bitmap_total(f.id_min, f.id_max, total)) {
        f.flags |= kPathWideIds;
        return f;
    }
    std::vector<uint32_t> bitmap((size_t)(path_bitmap_bytes_total(total) / 4), 0u);  // as the front allocates it
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < desc[b].L - 1; ++i) {  // the closing copy (the block's last city) sits out
            const unsigned long long bit =
                (unsigned long long)((long long)paths.at((size_t)desc[b].path + i).id - f.id_min);
            uint32_t &w = bitmap.at(bit >> 5);
            const uint32_t m = 1u << (bit & 31u);
            if (w & m) f.flags |= kPathDupId;
            w |= m;
        }
    return f;
}

// the ragged host front's scans (merge.hip: finite_cities, bbox_diagonal, host_fold_ok with lengths)
struct HostScan {
    bool finite, fold_ok;
    double dmax;
};
HostScan host_scan(const std::vector<tspgpu_city> &paths, const std::vector<BlockDesc> &desc)
{
    HostScan h{true, true, 0.0};
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (const tspgpu_city &c : paths) {
        if (!std::isfinite(c.x) || !std::isfinite(c.y)) h.finite = false;
        x0 = std::min(x0, c.x), x1 = std::max(x1, c.x), y0 = std::min(y0, c.y), y1 = std::max(y1, c.y);
    }
    h.dmax = path_bbox_diagonal(x0, x1, y0, y1);
    for (const BlockDesc &e : desc)
        if (e.L < 3) h.fold_ok = false;
    std::vector<int> ids;
    for (size_t b = 0; b < desc.size() && h.fold_ok; ++b) {
        const tspgpu_city *pb = &paths[(size_t)desc[b].path];
        if (pb[0].id != pb[desc[b].L - 1].id) h.fold_ok = false;
        for (int k = 0; k < desc[b].L - 1; ++k) ids.push_back(pb[k].id);
    }
    std::sort(ids.begin(), ids.end());
    if (h.fold_ok && std::adjacent_find(ids.begin(), ids.end()) != ids.end()) h.fold_ok = false;
    return h;
}

uint64_t bits_of(double v)
{
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    // the total-count forms give the uniform forms' values
    for (int B = 1; B < 40; ++B)
        for (int L = 2; L <= 21; ++L) {
            const unsigned long long t = (unsigned long long)B * L;
            CHECK(path_bitmap_bits_total(t) == path_bitmap_bits(B, L));
            CHECK(path_bitmap_bytes_total(t) == path_bitmap_bytes(B, L));
            CHECK(path_ids_fit_bitmap_total(-3, -3 + (long long)(8 * t) - 1, t) && !path_ids_fit_bitmap_total(-3, -3 + (long long)(8 * t), t));
        }
    long long cases = 0, folds = 0, wide = 0, dups = 0, opens = 0, last_bit = 0, partial_word = 0, twos = 0, mixed = 0;
    for (int round = 0; round < 4000; ++round) {
        const int B = 1 + (int)(rng() % 40);
        const int layout = (int)(rng() % 7);
        const bool with_twos = rng() % 4 == 0;  // 2-city blocks mixed in
        std::vector<int32_t> n(B);
        for (int b = 0; b < B; ++b) n[b] = with_twos && rng() % 3 == 0 ? 2 : 3 + (int)(rng() % 18);
        const std::vector<BlockDesc> desc = table_of(n);
        const int max_n = *std::max_element(n.begin(), n.end());
        const int stride = max_n + 1 + (int)(rng() % 3);
        const long long ncity = desc.back().city + n[B - 1];
        const unsigned long long total = (unsigned long long)(desc.back().path + desc.back().L);
        const int min_len = tour_len(*std::min_element(n.begin(), n.end()));
        std::vector<tspgpu_city> cities((size_t)ncity);
        std::uniform_real_distribution<double> u(-1000.0, 1000.0);
        const bool lattice = rng() % 3 == 0;
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n[b]; ++i) {
                const int g = (int)desc[b].city + i;  // the city's index in the packed array
                tspgpu_city &c = cities[(size_t)g];
                c.x = lattice ? (double)((int)(rng() % 5) - 2) : u(rng);
                c.y = lattice ? (double)((int)(rng() % 5) - 2) : u(rng);
                if (lattice && c.x == 0.0 && rng() % 2) c.x = -0.0;  // zeros of both signs
                if (lattice && c.y == 0.0 && rng() % 2) c.y = -0.0;
                switch (layout) {
                case 0: c.id = g; break;                               // dense
                case 1: c.id = 5; break;                               // all equal
                case 2: c.id = 1000000 * b + i; break;                 // spread past the bitmap
                case 3: c.id = INT_MIN + g; break;                     // dense at the bottom of the range
                case 6:  // the widest range that still fits: the last bit of the bitmap, often in a partial word
                    c.id = g == ncity - 1 ? -7 + (int)path_bitmap_bits_total(total) - 1 : -7 + g;
                    break;
                case 4: c.id = (b % 2 ? INT_MAX - g : INT_MIN + g); break;  // the whole int range
                default: c.id = g % std::max(2, (int)ncity - 1); break;     // one duplicate pair
                }
            }
        std::vector<int32_t> tour((size_t)B * stride, -1);
        for (int b = 0; b < B; ++b) {
            std::vector<int> perm(n[b] - 1);
            for (int i = 0; i < n[b] - 1; ++i) perm[i] = i + 1;
            std::shuffle(perm.begin(), perm.end(), rng);
            int32_t *row = &tour[(size_t)b * stride];
            if (n[b] == 2) {
                row[0] = 1, row[1] = 0;
            } else {
                row[0] = 0;
                for (int i = 0; i < n[b] - 1; ++i) row[1 + i] = perm[i];
                row[n[b]] = round % 17 == 3 && b == B / 2 ? 1 : 0;  // sometimes a path that does not close
            }
        }
        std::vector<tspgpu_city> paths;
        const PathFacts f = twin(cities, tour, stride, nullptr, desc, paths);
        const HostScan h = host_scan(paths, desc);
        ++cases;
        twos += min_len < 3;
        mixed += *std::min_element(n.begin(), n.end()) != max_n;
        CHECK(paths.size() == total);
        CHECK(path_facts_error(f) == 0 && h.finite);
        CHECK(bits_of(path_facts_diagonal(f)) == bits_of(h.dmax));
        const bool fold = path_facts_fold_ok_ragged(f, min_len);
        // the device rule may only be more careful than the sort: never "unique" where the host says no
        CHECK(!fold || h.fold_ok);
        if (!(f.flags & kPathWideIds)) CHECK(fold == h.fold_ok);
        CHECK(((f.flags & kPathWideIds) != 0) ==
              (min_len >= 3 && !path_ids_fit_bitmap_total(f.id_min, f.id_max, total)));
        if (min_len < 3) CHECK(!fold && !h.fold_ok);  // an open 2-city path: the general path on both sides
        if (layout == 6 && min_len >= 3) {
            CHECK(f.id_max - f.id_min == (long long)path_bitmap_bits_total(total) - 1 && !(f.flags & kPathWideIds));
            last_bit += 1, partial_word += total % 4 != 0;
        }
        folds += fold, wide += (f.flags & kPathWideIds) != 0, dups += (f.flags & kPathDupId) != 0;
        opens += (f.flags & kPathOpen) != 0;

        // errors: a status, a bad index, a non-finite coordinate
        if (round % 4 == 0 && B >= 3) {
            std::vector<int32_t> status(B, 0), t2 = tour;
            const int b1 = B / 3, b2 = B - 1;
            const int L1 = desc[b1].L;
            status[b1] = -ERANGE, status[b2] = -EINVAL;
            for (int i = 0; i < stride; ++i) t2[(size_t)b1 * stride + i] = 1 << 30;  // must not be read
            std::vector<tspgpu_city> p2;
            const PathFacts g = twin(cities, t2, stride, status.data(), desc, p2);
            CHECK(path_facts_error(g) == -ERANGE);
            CHECK(p2[(size_t)desc[b1].path].id == -12345);
            t2 = tour;
            t2[(size_t)b1 * stride + (L1 - 1)] = round % 8 ? n[b1] : -1;  // n_b itself is outside [0, n_b)
            const PathFacts g2 = twin(cities, t2, stride, nullptr, desc, p2);
            CHECK(path_facts_error(g2) == -EINVAL && (g2.flags & kPathBadIndex));
            CHECK(p2[(size_t)desc[b1].path].id == -12345);
            // an entry that is in range for a longer neighbour but not for this block
            if (n[b1] < max_n) {
                t2 = tour;
                t2[(size_t)b1 * stride] = max_n - 1;
                const PathFacts g4 = twin(cities, t2, stride, nullptr, desc, p2);
                CHECK(path_facts_error(g4) == -EINVAL && (g4.flags & kPathBadIndex));
            }
            std::vector<tspgpu_city> c2 = cities;
            c2[(size_t)desc[b2].city + 1].y = round % 8 ? NAN : INFINITY;
            const PathFacts g3 = twin(c2, tour, stride, nullptr, desc, p2);
            CHECK(path_facts_error(g3) == -EINVAL && (g3.flags & kPathNonFinite));
        }
    }
    CHECK(folds > 200 && wide > 200 && dups > 200 && opens > 200 && last_bit > 200 && partial_word > 100 &&
          twos > 200 && mixed > 3000);
    if (fails) {
        std::printf("check_paths_ragged: %d failures\n", fails);
        return 1;
    }
    std::printf("check_paths_ragged: ok (%lld cases: %lld fold_ok, %lld wide id ranges, %lld duplicates, %lld open "
                "paths, %lld id ranges ending on the bitmap's last bit, %lld of them in a partial word, %lld with "
                "2-city blocks, %lld with mixed sizes)\n",
                cases, folds, wide, dups, opens, last_bit, partial_word, twos, mixed);
    return 0;
}
