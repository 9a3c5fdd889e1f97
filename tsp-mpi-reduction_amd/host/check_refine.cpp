// The window plan of the refinement (csrc/refine_plan.h) against its
// definition, as a stand-alone host program (make check-refine builds it plain
// and under ASan + UBSan; tests/test_refine_plan.py runs both).
//
// Expectations are computed here on their own, by counting: window k of a
// pass exists iff its last position offset + k*(m+1) + m + 1 is inside the
// path.  Covered: m = 2..18, both offsets, L around every multiple of m+1 up
// to 6 windows, argument errors, strict limits, sizes past 2^31 elements, and
// the stop rule over every (max_passes, replaced history) up to 6 passes.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "refine_plan.h"

using namespace tspgpu;

static long cases = 0, windows_seen = 0;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "check_refine: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static void one(int64_t L, int m, int pass)
{
    RefinePass p;
    CHECK(refine_pass(L, m, pass, 0, &p) == 0);
    const int64_t o = (pass % 2) ? (m + 1) / 2 : 0;
    int64_t W = 0;
    while (o + W * (m + 1) + m + 1 <= L - 1) ++W;  // by counting
    CHECK(p.offset == o && p.windows == W && p.stride == m + 1 && p.w == m + 2);
    CHECK(p.cities == W * (m + 2) && p.dist == W * (m + 2) * (m + 2) && p.fold == W * (m + 1) * (m + 1));
    for (int64_t k = 0; k < W; ++k) {
        const int64_t s = p.offset + k * p.stride;
        CHECK(s >= 0 && s + p.w - 1 <= L - 1);            // inside the path
        if (k) CHECK(s == p.offset + (k - 1) * p.stride + p.w - 1);  // shares exactly its start with the one before
    }
    // the first position past the last window cannot start another
    CHECK(p.offset + W * p.stride + p.w - 1 > L - 1);
    ++cases;
    windows_seen += W;
}

// the stop rule, replayed: passes run for a history of per-pass replaced counts
static int passes_run(int max_passes, const int *replaced, int len)
{
    int64_t before = 0;
    for (int p = 0;; ++p) {
        const int64_t r = p < len ? replaced[p] : 0;
        if (refine_stop(p, max_passes, r, before)) return p + 1;
        before = r;
    }
}

int main()
{
    for (int m = kRefineMinM; m <= kRefineMaxM; ++m)
        for (int mult = 0; mult <= 6; ++mult)
            for (int d = -2; d <= (m + 1) / 2 + 2; ++d) {
                const int64_t L = (int64_t)mult * (m + 1) + d;
                if (L < 2) continue;
                for (int pass = 0; pass < 4; ++pass) one(L, m, pass);
            }
    RefinePass p;
    // argument errors
    CHECK(refine_pass(1, 7, 0, 0, &p) == -EINVAL && refine_pass(0, 7, 0, 0, &p) == -EINVAL);
    CHECK(refine_pass(100, 1, 0, 0, &p) == -EINVAL && refine_pass(100, 19, 0, 0, &p) == -EINVAL);
    CHECK(refine_pass(100, 7, -1, 0, &p) == -EINVAL && refine_pass(100, 7, 0, 0, nullptr) == -EINVAL);
    CHECK(refine_pass(100, 15, 0, 1, &p) == 0 && refine_pass(100, 16, 0, 1, &p) == -EINVAL);
    CHECK(refine_pass(100, 18, 0, 0, &p) == 0 && p.w == 20);
    // too short for a window: no error, no window
    CHECK(refine_pass(2, 2, 0, 0, &p) == 0 && p.windows == 0 && p.dist == 0);
    CHECK(refine_pass(3, 2, 1, 0, &p) == 0 && p.windows == 0);
    // 64-bit sizes: 10^7 cities at m = 18 pass 2^31 matrix elements
    CHECK(refine_pass(10000001, 18, 0, 0, &p) == 0);
    CHECK(p.windows == 10000000 / 19 && p.dist == p.windows * 400 && p.dist > (int64_t)1 << 27);
    CHECK(refine_pass((int64_t)2000000000, 2, 0, 0, &p) == 0 && p.dist == p.windows * 16 && p.dist > (int64_t)1 << 31);
    CHECK(refine_pass((int64_t)1 << 40, 2, 0, 0, &p) == -EINVAL);  // more windows than K1's int block count
    cases += 12;
    // the stop rule
    CHECK(refine_stop(0, 1, 5, 0));
    CHECK(!refine_stop(0, 2, 0, 0));  // pass 0 alone never stops a longer run
    CHECK(refine_stop(1, 8, 0, 0) && !refine_stop(1, 8, 1, 0) && !refine_stop(1, 8, 0, 1));
    {
        const int h0[] = {3, 2, 0, 0, 9, 9};
        CHECK(passes_run(8, h0, 6) == 4 && passes_run(3, h0, 6) == 3 && passes_run(1, h0, 6) == 1);
        const int h1[] = {0, 0};
        CHECK(passes_run(8, h1, 2) == 2);
        const int h2[] = {1, 0, 1, 0, 1, 0};
        CHECK(passes_run(6, h2, 6) == 6 && passes_run(9, h2, 6) == 7);
        // every history of 0/1 over 6 passes against the definition
        for (int bits = 0; bits < 64; ++bits)
            for (int mp = 1; mp <= 7; ++mp) {
                int h[6], want = mp;
                for (int i = 0; i < 6; ++i) h[i] = (bits >> i) & 1;
                for (int q = 1; q < mp; ++q) {
                    const int a = q < 6 ? h[q] : 0, b = q - 1 < 6 ? h[q - 1] : 0;
                    if (!a && !b) {
                        want = q + 1;
                        break;
                    }
                }
                CHECK(passes_run(mp, h, 6) == want);
                ++cases;
            }
    }
    std::printf("check_refine: ok (%ld cases, %ld windows)\n", cases, windows_seen);
    return 0;
}
