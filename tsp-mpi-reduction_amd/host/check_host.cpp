// Host-code check under AddressSanitizer + UBSan (`make check-asan`): the
// CPU halves of the product — the host parity layer (host/tsp_host.cpp:
// generator, distribution, mergeBlocks, reduction-tree replay) and K2's host
// algorithms (csrc/search_host.cpp: input check, multi-start tour, Lagrangian
// and 1-tree weights, the tie rule over the optimal set, the search's plan:
// seed depth and bound tables) — driven over a grid
// of sizes and edge cases, with the results compared against the CPU oracle
// (oracle/oracle.c, the checker, compiled into this test binary only).  Any
// sanitizer report aborts (-fno-sanitize-recover=all); a mismatch exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../oracle/oracle.h"
#include "../csrc/search_host.h"
#include "tsp_host.h"
#include "tspgpu.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int a = 0, int b = 0, int c = 0)
{
    if (!ok) {
        std::fprintf(stderr, "MISMATCH %s (%d %d %d)\n", what, a, b, c);
        ++failures;
    }
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
double urand()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) * 0x1p-53;
}

// generator, counts, merge tree: host layer == oracle for (n, B, P)
void check_pipeline(int n, int B, int P)
{
    std::vector<tspgpu_city> h((size_t)n * B);
    std::vector<oracle_city> o((size_t)n * B);
    tsphost_generate(n, B, 1000, 1000, h.data());
    oracle_generate(n, B, 1000, 1000, o.data());
    for (size_t i = 0; i < h.size(); ++i)
        expect(h[i].id == o[i].id && h[i].x == o[i].x && h[i].y == o[i].y, "generate", n, B, (int)i);
    std::vector<int> ch(P), co(P);
    tsphost_distribution_counts(B, P, ch.data());
    oracle_distribution_counts(B, P, co.data());
    expect(ch == co, "distribution counts", B, P);
    // every block solved by the oracle, then the host layer's fold + tree
    const int L = n == 2 ? 2 : n + 1;  // tspgpu_tour_length (the n = 2 quirk, tsp.cpp:483-502)
    std::vector<tspgpu_city> paths((size_t)B * L);
    std::vector<double> costs(B);
    std::vector<double> d((size_t)n * n);
    std::vector<int32_t> tour(n + 1);
    for (int b = 0; b < B; ++b) {
        oracle_distance_matrix(&o[(size_t)b * n], n, d.data());
        oracle_solve_block(d.data(), n, &costs[b], tour.data());
        for (int i = 0; i < L; ++i) paths[(size_t)b * L + i] = h[(size_t)b * n + tour[i]];
    }
    double fh = 0.0, fo = 0.0;
    std::vector<char> lh(1 << 16), lo(1 << 16);
    const int rh = tsphost_reduce(paths.data(), L, costs.data(), B, P, &fh, lh.data(), (int)lh.size());
    const int ro = oracle_pipeline(n, B, 1000, 1000, P, &fo, lo.data(), (int)lo.size());
    expect(rh == ro, "reduce rc", n, B, P);
    if (rh == 0 && ro == 0) {
        expect(fh == fo, "reduce final cost", n, B, P);
        expect(std::strcmp(lh.data(), lo.data()) == 0, "reduce log", n, B, P);
    }
}

// mergeBlocks on two random closed paths
void check_merge(int L1, int L2)
{
    std::vector<tspgpu_city> a(L1), b(L2);
    std::vector<oracle_city> oa(L1), ob(L2);
    for (int i = 0; i < L1; ++i) a[i] = {i, 1000 * urand(), 1000 * urand()};
    for (int i = 0; i < L2; ++i) b[i] = {100 + i, 1000 * urand(), 1000 * urand()};
    a[L1 - 1] = a[0];
    b[L2 - 1] = b[0];
    for (int i = 0; i < L1; ++i) oa[i] = {a[i].id, a[i].x, a[i].y};
    for (int i = 0; i < L2; ++i) ob[i] = {b[i].id, b[i].x, b[i].y};
    std::vector<tspgpu_city> out(L1 + L2 - 1);
    std::vector<oracle_city> oout(L1 + L2 - 1);
    double ch = 0.0, co = 0.0;
    const int rh = tsphost_merge(a.data(), L1, 10.0, b.data(), L2, 20.0, out.data(), &ch);
    const int ro = oracle_merge_blocks(oa.data(), L1, 10.0, ob.data(), L2, 20.0, oout.data(), &co);
    expect(rh == ro || rh < 0, "merge length", L1, L2);
    if (rh == ro && rh > 0) {
        expect(ch == co, "merge cost", L1, L2);
        for (int i = 0; i < rh; ++i) expect(out[i].id == oout[i].id, "merge path", L1, L2, i);
    }
}

int tree_tables = 0;  // tree tables check_bound_tables saw (main: some must have been built)

// build_bound_tables (csrc/search_host.cpp) against the tables' definitions;
// d = the f64 view of dist.  A bound that is not a lower bound prunes the
// optimum, so for n <= 12 the sums are compared with the oracle's optimum —
// exactly: each entry is rounded DOWN by a margin far above the sums' rounding.
void check_bound_tables(const void *dist, int dtype, int n, const std::vector<double> &d)
{
    using namespace tspgpu::host;
    const bool integer = dtype == TSPGPU_I32;
    bool sym = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) sym = sym && d[(size_t)i * n + j] == d[(size_t)j * n + i];
    expect(is_symmetric(dist, dtype, n) == sym, "is_symmetric", n, integer);
    double opt = 0.0;
    if (n <= 12) {
        std::vector<int32_t> ot(n + 1);
        oracle_solve_block(d.data(), n, &opt, ot.data());
    }
    // the default knobs, no Lagrangian weights, and the tree bound from 2 cities left
    for (int cfg = 0; cfg < 3; ++cfg) {
        PlanOptions o;
        if (cfg == 1) o.use_lagrange = false;
        if (cfg == 2) o.mst_min_rem = 2;
        const SeedPlan plan = plan_seeds(n, 0, 1, 0, (uint64_t)256 * 8 * 256, 256, o, sym, false);
        BoundTables t;
        build_bound_tables(dist, dtype, n, sym, plan, o, t);
        expect(t.sym == (sym ? 1 : 0), "tables sym", n, integer, cfg);
        double asum = 0.0;
        for (int x = 0; x < n; ++x) {
            double m = INFINITY;
            for (int i = 0; i < n; ++i)
                if (i != x) m = std::fmin(m, d[(size_t)i * n + x]);
            if (integer) {
                expect((int)t.amin_i.size() == n && (double)t.amin_i[x] == m, "amin i32", n, x, cfg);
                asum += t.amin_i[x];
            } else {
                const double a = (int)t.amin_d.size() == n ? t.amin_d[x] : -1.0, g = std::ldexp(a, 20);
                expect(g == std::floor(g) && m - a >= 0.0 && m - a < 0x1p-20, "amin f64 grid", n, x, cfg);
                asum += a;
            }
        }
        if (n <= 12) expect(asum <= opt, "sum of amin <= optimum", n, integer, cfg);
        if (!sym) {
            expect(t.bnd2_d.empty() && t.bnd2_i.empty() && t.mt.empty() && !t.mst_on, "asymmetric: no bnd2, no tree", n,
                   integer, cfg);
            continue;
        }
        expect((integer ? t.bnd2_i.size() : t.bnd2_d.size()) == (size_t)2 * n, "bnd2 size", n, integer, cfg);
        if (n <= 12) {
            double bsum = 0.0;
            for (int x = 0; x < n; ++x) bsum += integer ? (double)t.bnd2_i[2 * x] : t.bnd2_d[2 * x];
            expect(bsum <= opt, "sum of b <= optimum", n, integer, cfg);
        }
        expect(t.mst_on == !t.mt.empty(), "tree flag", n, integer, cfg);
        if (!t.mst_on) continue;
        ++tree_tables;
        expect(t.mt.size() == (size_t)n * n + n + 1, "tree size", n, integer, cfg);
        const double *pi = t.mt.data() + (size_t)n * n;
        const double mg = t.mt[(size_t)n * n + n];
        for (int x = 0; x < n; ++x)
            for (int y = 0; y < n; ++y) {
                const double v = d[(size_t)x * n + y] + pi[x] + pi[y], w = t.mt[(size_t)x * n + y];
                expect(std::memcmp(&v, &w, 8) == 0, "tree d'", n, x, y);
                // symmetric up to the two summation orders: fl(fl(d + pi_x) + pi_y)
                // and fl(fl(d + pi_y) + pi_x) each lie within (2u + u^2) S of the real
                // sum, S = |d| + |pi_x| + |pi_y|, u = 2^-53, so they differ by less
                // than 8u S (measured: up to 2.1u S, on one pair in five) — and by
                // less than the table's margin, which is what covers it on the device
                const double S = std::fabs(d[(size_t)x * n + y]) + std::fabs(pi[x]) + std::fabs(pi[y]);
                const double asym = std::fabs(w - t.mt[(size_t)y * n + x]);
                expect(asym <= 0x1p-50 * S && asym < mg, "tree symmetric", n, x, y);
            }
        expect(std::isfinite(mg) && mg > 0.0, "tree margin", n, integer, cfg);
    }
}

// K2 host algorithms on random instances: the multi-start tour is a
// permutation whose cost is its left fold, >= the optimum; the tie rule on the
// optimal tour alone returns that tour; the weights are finite
void check_search_host(int n, bool integer)
{
    std::vector<double> xy(2 * n);
    for (auto &v : xy) v = 1000 * urand();
    std::vector<double> d((size_t)n * n);
    std::vector<int32_t> di((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            d[(size_t)i * n + j] = std::sqrt(std::pow(xy[2 * i] - xy[2 * j], 2) + std::pow(xy[2 * i + 1] - xy[2 * j + 1], 2));
            di[(size_t)i * n + j] = (int32_t)std::lround(d[(size_t)i * n + j]);
            if (integer) d[(size_t)i * n + j] = di[(size_t)i * n + j];
        }
    const void *dist = integer ? (const void *)di.data() : (const void *)d.data();
    const int dtype = integer ? TSPGPU_I32 : TSPGPU_F64;
    expect(tspgpu::host::validate_search(dist, dtype, n) == 0, "validate", n);
    std::vector<int32_t> t(n + 1);
    double ub = 0.0;
    expect(tspgpu_heuristic_tour(dist, dtype, n, &ub, t.data()) == 0, "heuristic rc", n);
    std::vector<int> seen(n, 0);
    double fold = 0.0;
    for (int i = 0; i < n; ++i) {
        seen[t[i]]++;
        fold = fold + d[(size_t)t[i] * n + t[i + 1]];
    }
    for (int i = 0; i < n; ++i) expect(seen[i] == 1, "heuristic permutation", n, i);
    expect(t[0] == 0 && t[n] == 0 && fold == ub, "heuristic cost", n);
    double ub2 = 0.0;
    expect(tspgpu_heuristic_tour_starts(dist, dtype, n, 1, 3, &ub2, nullptr) == 0 && ub2 >= 0.0, "starts", n);
    std::vector<double> pi;
    tspgpu::host::lagrange_pi(d, n, pi);
    for (double v : pi) expect(std::isfinite(v), "lagrange finite", n);
    tspgpu::host::held_karp_pi(d, n, pi);
    for (double v : pi) expect(std::isfinite(v), "held-karp finite", n);
    if (n <= 12) {  // the exact optimum (oracle DP) as the only record
        double opt = 0.0;
        std::vector<int32_t> ot(n + 1);
        oracle_solve_block(d.data(), n, &opt, ot.data());
        expect(opt <= ub, "bound above optimum", n);
        tspgpu_tour_record r{};
        uint64_t bits = 0;
        if (integer) {
            bits = (uint32_t)(int32_t)opt;
        } else {
            std::memcpy(&bits, &opt, 8);
        }
        r.cost = bits;
        for (int i = 1; i < n; ++i) r.city[i - 1] = (uint8_t)ot[i];
        std::vector<int32_t> sel(n + 1);
        expect(tspgpu_select_tour(dist, dtype, n, &r, 1, bits, sel.data()) == 0, "select rc", n);
        expect(sel == ot, "select tour", n);
    }
    // invalid inputs are refused, not read out of bounds
    expect(tspgpu::host::validate_search(dist, dtype, 2) != 0, "validate n=2", n);
    expect(tspgpu_select_tour(dist, dtype, n, nullptr, 0, 0, t.data()) != 0, "select empty", n);
    // the bound tables of the search's plan: as generated (symmetric), then
    // with one entry raised (asymmetric)
    check_bound_tables(dist, dtype, n, d);
    d[1 * n + 2] += 3.0;
    di[1 * n + 2] += 3;
    check_bound_tables(dist, dtype, n, d);
}

// plan_seeds over sizes, shard counts and requested depths (256 CUs, 8 blocks
// of 256 lanes per CU): depth within 1..N-1, items = N(N-1)..(N-depth+1) below
// 2^31 and split over the shards without loss, a frontier only with levels to
// expand, a requested depth honoured up to the clamps
void check_plan_seeds(int n)
{
    using namespace tspgpu::host;
    const int N = n - 1, cus = 256;
    const uint64_t lanes = (uint64_t)cus * 8 * 256;
    const PlanOptions o;
    for (int nshards : {1, 2, 3, 8})
        for (int req : {0, 1, 3})
            for (int variant = 0; variant < 4; ++variant) {
                const bool symmetric = variant & 1, enum_shard = variant & 2;
                uint64_t sum = 0, items = 0;
                for (int shard = 0; shard < nshards; ++shard) {
                    const SeedPlan p = plan_seeds(n, shard, nshards, req, lanes, cus, o, symmetric, enum_shard);
                    expect(p.depth >= 1 && p.depth <= N - 1, "plan depth range", n, nshards, req);
                    uint64_t f = 1;
                    for (int l = 0; l < p.depth; ++l) f *= (uint64_t)(N - l);
                    expect(p.items == f && f < (1ull << 31), "plan items", n, nshards, req);
                    expect(!p.frontier || (N - o.tail_len > p.depth && !enum_shard), "plan frontier", n, nshards, req);
                    // (N <= 31: a depth of 3 is below 2^31 prefixes, so only N - 1 clamps it)
                    if (req > 0) expect(p.depth == (req < N - 1 ? req : N - 1), "plan requested depth", n, nshards, req);
                    sum += p.local_items;
                    items = p.items;
                }
                expect(sum == items, "plan shard split", n, nshards, req);
            }
}

}  // namespace

int main()
{
    for (int n : {2, 3, 5, 8, 12})
        for (int B : {1, 2, 4, 7, 16})
            for (int P : {1, 2, 3, 4, 8})
                if (B >= P) check_pipeline(n, B, P);
    for (int L1 : {3, 5, 9, 17})
        for (int L2 : {3, 6, 13}) check_merge(L1, L2);
    for (int n = 3; n <= 32; n += (n < 12 ? 1 : 5))
        for (bool integer : {false, true}) check_search_host(n, integer);
    expect(tree_tables > 0, "no tree table was built");
    for (int n = 4; n <= 32; ++n) check_plan_seeds(n);
    std::printf("check_host: %s (%d mismatches)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
