// The host plan of the 2-opt stage (csrc/two_opt_plan.h) against its
// definition, as a stand-alone host program (make check-two-opt builds it
// plain and under ASan + UBSan; tests/test_two_opt_plan.py runs both).
//
// The grid size is checked against its defining inequality.  The selection is
// checked against a quadratic restatement (a stable insertion order and a
// scan over every accepted range) on random range sets and on the adversarial
// ones: all nested, chains that share an edge, chains that only touch, equal
// gains, single candidates, none.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "two_opt_plan.h"

using namespace tspgpu;

static long cases = 0, moves_seen = 0;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "check_two_opt: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

// the definition: repeatedly take the best remaining candidate by (gain
// descending, i ascending); accept it iff no accepted range shares an edge
static void restated(std::vector<TwoOptCand> c, std::vector<TwoOptCand> *acc, double *gain)
{
    while (!c.empty()) {
        size_t b = 0;
        for (size_t k = 1; k < c.size(); ++k)
            if (c[k].gain > c[b].gain || (c[k].gain == c[b].gain && c[k].i < c[b].i)) b = k;
        bool ok = true;
        for (const TwoOptCand &a : *acc)
            if (!(c[b].j < a.i || a.j < c[b].i)) ok = false;
        if (ok) {
            acc->push_back(c[b]);
            *gain = *gain + c[b].gain;
        }
        c.erase(c.begin() + (long)b);
    }
}

static void one(const std::vector<TwoOptCand> &in, int64_t L)
{
    std::vector<TwoOptCand> want;
    double want_gain = 0.25;  // (the fold starts from what the caller holds)
    restated(in, &want, &want_gain);
    std::vector<TwoOptCand> c = in;
    const size_t n = c.size();
    std::vector<int32_t> ai(n + 1, -7), aj(n + 1, -7), pre(n + 2, -7);
    double gain = 0.25;
    const int64_t m = two_opt_select(c.data(), (int64_t)n, L, ai.data(), aj.data(), pre.data(), &gain);
    CHECK(m == (int64_t)want.size());
    CHECK(gain == want_gain);
    CHECK(pre[0] == 0);
    for (int64_t k = 0; k < m; ++k) {
        CHECK(ai[k] == want[k].i && aj[k] == want[k].j);
        CHECK(pre[k + 1] == pre[k] + (aj[k] - ai[k]) / 2);
    }
    CHECK(ai[m] == -7 && aj[m] == -7 && pre[m + 1] == -7);  // nothing written past the accepted
    CHECK((n == 0) == (m == 0));                            // the best candidate is always accepted
    ++cases;
    moves_seen += m;
}

// n candidates on distinct positions inside L
static std::vector<TwoOptCand> random_set(int n, int L, int max_len, bool few_gains)
{
    std::vector<TwoOptCand> c;
    std::vector<char> used((size_t)L, 0);
    for (int k = 0; k < n; ++k) {
        const int i = (int)(rnd() % (uint64_t)(L - 3));
        if (used[i]) continue;
        used[i] = 1;
        int j = i + 2 + (int)(rnd() % (uint64_t)max_len);
        if (j > L - 2) j = L - 2;
        const double g = few_gains ? 1.0 + (double)(rnd() % 3) : 1e-3 + (double)(rnd() % 1000003) / 7.0;
        c.push_back({g, i, j});
    }
    return c;
}

int main()
{
    // the grid: the largest g with 2 g g <= L, within [1, 2048]
    for (int64_t L = 1; L <= 70000; ++L) {
        const int g = two_opt_grid(L);
        CHECK(g >= 1 && (g == 1 || 2 * (int64_t)g * g <= L) && 2 * (int64_t)(g + 1) * (g + 1) > L);
        ++cases;
    }
    CHECK(two_opt_grid(1) == 1 && two_opt_grid(7) == 1 && two_opt_grid(8) == 2 && two_opt_grid(17) == 2);
    CHECK(two_opt_grid(18) == 3 && two_opt_grid(262145) == 362 && two_opt_grid(2 * 2048 * 2048 - 1) == 2047);
    CHECK(two_opt_grid(2 * 2048 * 2048) == 2048 && two_opt_grid(kTwoOptMaxL) == 2048);
    // random sets: short and long ranges, distinct and repeated gains
    for (int rep = 0; rep < 400; ++rep) {
        const int L = 8 + (int)(rnd() % 400);
        one(random_set(1 + (int)(rnd() % 120), L, 1 + (int)(rnd() % 6), rep % 2), L);
        one(random_set(1 + (int)(rnd() % 120), L, L, rep % 3 == 0), L);
    }
    // nothing, one
    one({}, 100);
    one({{2.5, 0, 2}}, 4);
    one({{2.5, 3, 98}}, 100);
    // all nested, best outermost / innermost / in the middle
    for (int mode = 0; mode < 3; ++mode) {
        std::vector<TwoOptCand> c;
        for (int k = 0; k < 40; ++k) {
            const double g = mode == 0 ? 100.0 - k : (mode == 1 ? 1.0 + k : 50.0 - (k - 20) * (k - 20));
            c.push_back({g + 1000.0, k, 198 - k});
        }
        one(c, 200);
    }
    // chains: (i, j) then (j, j') share edge j, (i, j) then (j+1, j') only touch
    for (int share = 0; share < 2; ++share)
        for (int order = 0; order < 3; ++order) {
            std::vector<TwoOptCand> c;
            int at = 0;
            for (int k = 0; k < 50; ++k) {
                const int len = 2 + k % 4;
                const double g = order == 0 ? 1.0 + k : (order == 1 ? 100.0 - k : 1.0 + (k * 37) % 50);
                c.push_back({g, at, at + len});
                at += len + (share ? 0 : 1);
            }
            one(c, at + 2);
        }
    // equal gains everywhere: i ascending decides
    {
        std::vector<TwoOptCand> c;
        for (int k = 0; k < 60; ++k) c.push_back({3.0, 59 - k, 59 - k + 2 + k % 5});
        one(c, 200);
    }
    // refused inputs: nothing is accepted from them
    {
        int32_t ai[4], aj[4], pre[5];
        double gain = 0.0;
        TwoOptCand bad[2] = {{1.0, 0, 2}, {1.0, 5, 9}};
        CHECK(two_opt_select(bad, 2, 11, ai, aj, pre, &gain) == 2);
        CHECK(two_opt_select(bad, 2, 10, ai, aj, pre, &gain) == -EINVAL);  // j > L - 2
        CHECK(two_opt_select(bad, -1, 11, ai, aj, pre, &gain) == -EINVAL);
        CHECK(two_opt_select(nullptr, 2, 11, ai, aj, pre, &gain) == -EINVAL);
        CHECK(two_opt_select(bad, 2, 11, ai, aj, nullptr, &gain) == -EINVAL);
        CHECK(two_opt_select(bad, 2, 11, ai, aj, pre, nullptr) == -EINVAL);
        CHECK(two_opt_select(nullptr, 0, 11, nullptr, nullptr, pre, &gain) == 0 && pre[0] == 0);
        TwoOptCand neg[1] = {{-1.0, 0, 2}}, zero[1] = {{0.0, 0, 2}}, shortj[1] = {{1.0, 4, 5}}, negi[1] = {{1.0, -1, 2}};
        CHECK(two_opt_select(neg, 1, 11, ai, aj, pre, &gain) == -EINVAL);
        CHECK(two_opt_select(zero, 1, 11, ai, aj, pre, &gain) == -EINVAL);
        CHECK(two_opt_select(shortj, 1, 11, ai, aj, pre, &gain) == -EINVAL);
        CHECK(two_opt_select(negi, 1, 11, ai, aj, pre, &gain) == -EINVAL);
        TwoOptCand twice[2] = {{1.0, 3, 5}, {1.0, 3, 6}};
        CHECK(two_opt_select(twice, 2, 11, ai, aj, pre, &gain) == -EINVAL);
        cases += 12;
    }
    std::printf("check_two_opt: ok (%ld cases, %ld moves)\n", cases, moves_seen);
    return 0;
}
