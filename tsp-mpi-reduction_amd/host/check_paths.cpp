// The host side of the K1 -> K3 hand-off (csrc/paths_facts.h) without a GPU:
// a host twin of the device summary and of the bitmap rule (the same order
// keys, extrema, flags and atomicOr bitmap, run serially) against the scans
// the host front of tspgpu_reduce does (std::min / std::max over the cities,
// a sort of every id).  Checked: the keys are monotone and round-trip; the
// diagonal from the keys has the bits of the direct scan's, zeros of both
// signs included; the bitmap decides uniqueness exactly when the id range
// fits, and raises kPathWideIds (never a wrong "unique") when it does not;
// statuses, bad indices and non-finite coordinates fail with the documented
// codes and a bad block's row is never read; no index leaves its array, the
// bitmap's last bit in a partial 32-bit word included (the program runs under
// ASan + UBSan too: `make check-paths`).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

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

// what paths_gather_kernel and paths_unique_kernel compute, serially
PathFacts twin(const std::vector<tspgpu_city> &cities, const std::vector<int32_t> &tour, const int32_t *status, int n,
               int B, std::vector<tspgpu_city> &paths)
{
    const int L = tour_len(n);
    PathFacts f = path_facts_init();
    paths.assign((size_t)B * L, tspgpu_city{-12345, -1.0, -1.0});
    for (int b = 0; b < B; ++b) {
        if (status && status[b] != 0) {
            const unsigned long long w = ((unsigned long long)b << 32) | (unsigned)status[b];
            f.first_bad = std::min(f.first_bad, w);
            continue;  // the row is never read
        }
        bool rowbad = false;
        for (int i = 0; i < L; ++i) {
            const int t = tour.at((size_t)b * (n + 1) + i);
            if (t < 0 || t >= n) rowbad = true;
        }
        if (rowbad) {
            f.flags |= kPathBadIndex;
            continue;
        }
        for (int i = 0; i < L; ++i) {
            const tspgpu_city c = cities.at((size_t)b * n + tour[(size_t)b * (n + 1) + i]);
            paths.at((size_t)b * L + i) = c;
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
        if (paths[(size_t)b * L + L - 1].id != paths[(size_t)b * L].id) f.flags |= kPathOpen;
    }
    if (L < 3 || f.first_bad != ~0ull || (f.flags & kPathBadIndex)) return f;
    if (!path_ids_fit_bitmap(f.id_min, f.id_max, B, L)) {
        f.flags |= kPathWideIds;
        return f;
    }
    std::vector<uint32_t> bitmap((size_t)(path_bitmap_bytes(B, L) / 4), 0u);  // as the front allocates it
    for (size_t k = 0; k < paths.size(); ++k) {
        if (k % L == (size_t)L - 1) continue;
        const unsigned long long bit = (unsigned long long)((long long)paths[k].id - f.id_min);
        uint32_t &w = bitmap.at(bit >> 5);
        const uint32_t m = 1u << (bit & 31u);
        if (w & m) f.flags |= kPathDupId;
        w |= m;
    }
    return f;
}

// the host front's scans (merge.hip: finite_cities, bbox_diagonal, the id sort)
struct HostScan {
    bool finite, fold_ok;
    double dmax;
};
HostScan host_scan(const std::vector<tspgpu_city> &paths, int L, int B)
{
    HostScan h{true, L >= 3, 0.0};
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (const tspgpu_city &c : paths) {
        if (!std::isfinite(c.x) || !std::isfinite(c.y)) h.finite = false;
        x0 = std::min(x0, c.x), x1 = std::max(x1, c.x), y0 = std::min(y0, c.y), y1 = std::max(y1, c.y);
    }
    h.dmax = path_bbox_diagonal(x0, x1, y0, y1);
    std::vector<int> ids;
    for (int b = 0; b < B && h.fold_ok; ++b) {
        if (paths[(size_t)b * L].id != paths[(size_t)b * L + L - 1].id) h.fold_ok = false;
        for (int k = 0; k < L - 1; ++k) ids.push_back(paths[(size_t)b * L + k].id);
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
    std::mt19937_64 rng(20261020);
    // keys: monotone, round trip, sentinels free
    {
        std::vector<double> v = {-INFINITY, -1e308, -2.5, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.5, 1e308, INFINITY};
        std::uniform_real_distribution<double> u(-1e6, 1e6);
        for (int i = 0; i < 100000; ++i) v.push_back(u(rng));
        std::sort(v.begin(), v.end(), [](double a, double b) { return a < b || (a == b && std::signbit(a) > std::signbit(b)); });
        for (size_t i = 0; i < v.size(); ++i) {
            const unsigned long long k = path_order_key(v[i]);
            CHECK(bits_of(path_key_value(k)) == bits_of(v[i]));
            CHECK(k != 0ull && k != ~0ull);
            if (i) CHECK(v[i - 1] < v[i] ? path_order_key(v[i - 1]) < k : path_order_key(v[i - 1]) <= k);
        }
    }
    long long cases = 0, folds = 0, wide = 0, dups = 0, opens = 0, last_bit = 0, partial_word = 0;
    for (int round = 0; round < 4000; ++round) {
        const int n = 2 + (int)(rng() % 19), B = 1 + (int)(rng() % 40), L = tour_len(n);
        const int layout = (int)(rng() % 7);
        std::vector<tspgpu_city> cities((size_t)B * n);
        std::uniform_real_distribution<double> u(-1000.0, 1000.0);
        const bool lattice = rng() % 3 == 0;
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n; ++i) {
                tspgpu_city &c = cities[(size_t)b * n + i];
                c.x = lattice ? (double)((int)(rng() % 5) - 2) : u(rng);
                c.y = lattice ? (double)((int)(rng() % 5) - 2) : u(rng);
                if (lattice && c.x == 0.0 && rng() % 2) c.x = -0.0;  // zeros of both signs
                if (lattice && c.y == 0.0 && rng() % 2) c.y = -0.0;
                switch (layout) {
                case 0: c.id = b * n + i; break;                          // dense
                case 1: c.id = 5; break;                                  // all equal
                case 2: c.id = 1000000 * b + i; break;                    // spread past the bitmap
                case 3: c.id = INT_MIN + b * n + i; break;                // dense at the bottom of the range
                case 6:  // the widest range that still fits: the last bit of the bitmap, often in a partial word
                    c.id = b * n + i == B * n - 1 ? -7 + (int)path_bitmap_bits(B, L) - 1 : -7 + b * n + i;
                    break;
                case 4: c.id = (b % 2 ? INT_MAX - b * n - i : INT_MIN + b * n + i); break;  // the whole int range
                default: c.id = (b * n + i) % std::max(2, B * n - 1); break;  // one duplicate pair
                }
            }
        std::vector<int32_t> tour((size_t)B * (n + 1), -1);
        for (int b = 0; b < B; ++b) {
            std::vector<int> perm(n - 1);
            for (int i = 0; i < n - 1; ++i) perm[i] = i + 1;
            std::shuffle(perm.begin(), perm.end(), rng);
            int32_t *row = &tour[(size_t)b * (n + 1)];
            if (n == 2) {
                row[0] = 1, row[1] = 0;
            } else {
                row[0] = 0;
                for (int i = 0; i < n - 1; ++i) row[1 + i] = perm[i];
                row[n] = round % 17 == 3 && b == B / 2 ? 1 : 0;  // sometimes a path that does not close
            }
        }
        std::vector<tspgpu_city> paths;
        const PathFacts f = twin(cities, tour, nullptr, n, B, paths);
        const HostScan h = host_scan(paths, L, B);
        ++cases;
        CHECK(path_facts_error(f) == 0 && h.finite);
        CHECK(bits_of(path_facts_diagonal(f)) == bits_of(h.dmax));
        const bool fold = path_facts_fold_ok(f, L);
        // the device rule may only be more careful than the sort: never "unique" where the host says no
        CHECK(!fold || h.fold_ok);
        if (!(f.flags & kPathWideIds)) CHECK(fold == h.fold_ok);
        CHECK(((f.flags & kPathWideIds) != 0) == (L >= 3 && !path_ids_fit_bitmap(f.id_min, f.id_max, B, L)));
        if (layout == 6 && L >= 3) {
            CHECK(f.id_max - f.id_min == (long long)path_bitmap_bits(B, L) - 1 && !(f.flags & kPathWideIds));
            last_bit += 1, partial_word += (B * L) % 4 != 0;
        }
        folds += fold, wide += (f.flags & kPathWideIds) != 0, dups += (f.flags & kPathDupId) != 0;
        opens += (f.flags & kPathOpen) != 0;

        // errors: a status, a bad index, a non-finite coordinate
        if (round % 4 == 0 && B >= 3) {
            std::vector<int32_t> status(B, 0), t2 = tour;
            const int b1 = B / 3, b2 = B - 1;
            status[b1] = -ERANGE, status[b2] = -EINVAL;
            for (int i = 0; i <= n; ++i) t2[(size_t)b1 * (n + 1) + i] = 1 << 30;  // must not be read
            std::vector<tspgpu_city> p2;
            const PathFacts g = twin(cities, t2, status.data(), n, B, p2);
            CHECK(path_facts_error(g) == -ERANGE);
            CHECK(p2[(size_t)b1 * L].id == -12345);
            t2 = tour;
            t2[(size_t)b1 * (n + 1) + (L - 1)] = round % 8 ? n : -1;
            const PathFacts g2 = twin(cities, t2, nullptr, n, B, p2);
            CHECK(path_facts_error(g2) == -EINVAL && (g2.flags & kPathBadIndex));
            CHECK(p2[(size_t)b1 * L].id == -12345);
            std::vector<tspgpu_city> c2 = cities;
            c2[(size_t)b2 * n + 1].y = round % 8 ? NAN : INFINITY;
            const PathFacts g3 = twin(c2, tour, nullptr, n, B, p2);
            CHECK(path_facts_error(g3) == -EINVAL && (g3.flags & kPathNonFinite));
        }
    }
    CHECK(folds > 200 && wide > 200 && dups > 200 && opens > 20 && last_bit > 200 && partial_word > 100);
    if (fails) {
        std::printf("check_paths: %d failures\n", fails);
        return 1;
    }
    std::printf("check_paths: ok (%lld cases: %lld fold_ok, %lld wide id ranges, %lld duplicates, %lld open paths, "
                "%lld id ranges ending on the bitmap's last bit, %lld of them in a partial word)\n",
                cases, folds, wide, dups, opens, last_bit, partial_word);
    return 0;
}
