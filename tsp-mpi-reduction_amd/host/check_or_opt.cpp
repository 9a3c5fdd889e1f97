// The host plan of the Or-opt stage (csrc/or_opt_plan.h) against its
// definition, as a stand-alone host program (make check-or-opt builds it plain
// and under ASan + UBSan; tests/test_or_opt_plan.py runs both).
//
// The selection is checked against a quadratic restatement (take the best
// remaining candidate, scan every accepted range) on random candidate sets
// and on the adversarial ones: all nested, chains that share an edge, chains
// that only touch, equal gains, the same move reported by both of its ends,
// forward and backward moves over one range, single candidates, none; then
// every way a candidate can lie outside the contract.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "or_opt_plan.h"

using namespace tspgpu;

static long cases = 0, moves_seen = 0;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "check_or_opt: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

struct Range {
    int32_t lo, hi, how;
};

// the contract's range and rotation of one move
static Range range_of(const OrOptCand &c)
{
    const int32_t k = c.kr & 3, h = c.a + k - 1;
    if (c.t > h) return {c.a - 1, c.t, c.kr | kOrOptFwd};
    return {c.t, h, c.kr};
}

// the definition: repeatedly take the best remaining candidate by (gain
// descending, s ascending); accept it iff no accepted range shares an edge
static void restated(std::vector<OrOptCand> c, std::vector<Range> *acc, double *gain)
{
    while (!c.empty()) {
        size_t b = 0;
        for (size_t k = 1; k < c.size(); ++k)
            if (c[k].gain > c[b].gain || (c[k].gain == c[b].gain && c[k].s < c[b].s)) b = k;
        const Range r = range_of(c[b]);
        bool ok = true;
        for (const Range &a : *acc)
            if (!(r.hi < a.lo || a.hi < r.lo)) ok = false;
        if (ok) {
            acc->push_back(r);
            *gain = *gain + c[b].gain;
        }
        c.erase(c.begin() + (long)b);
    }
}

static void one(const std::vector<OrOptCand> &in, int64_t L, int max_seg = 3)
{
    std::vector<Range> want;
    double want_gain = 0.25;  // (the fold starts from what the caller holds)
    restated(in, &want, &want_gain);
    std::vector<OrOptCand> c = in;
    const size_t n = c.size();
    std::vector<int32_t> lo(n + 1, -7), hi(n + 1, -7), how(n + 1, -7), pre(n + 2, -7);
    double gain = 0.25;
    const int64_t m = or_opt_select(c.data(), (int64_t)n, L, max_seg, lo.data(), hi.data(), how.data(), pre.data(), &gain);
    CHECK(m == (int64_t)want.size());
    CHECK(gain == want_gain);
    CHECK(pre[0] == 0);
    for (int64_t k = 0; k < m; ++k) {
        CHECK(lo[k] == want[k].lo && hi[k] == want[k].hi && how[k] == want[k].how);
        CHECK(pre[k + 1] == pre[k] + (hi[k] - lo[k]));
        CHECK(hi[k] - lo[k] > (how[k] & 3) && lo[k] >= 0 && hi[k] <= L - 2);  // a rotation inside the path
    }
    CHECK(m <= L / 3);
    CHECK(lo[m] == -7 && hi[m] == -7 && how[m] == -7 && pre[m + 1] == -7);  // nothing written past the accepted
    CHECK((n == 0) == (m == 0));                                           // the best candidate is always accepted
    ++cases;
    moves_seen += m;
}

static OrOptCand cand(double gain, int a, int k, int t, int rev, bool at_last = false)
{
    return {gain, at_last ? a + k - 1 : a, a, t, or_opt_kr(k, rev)};
}

// n candidates on distinct positions inside L; the insertion at most max_far edges away
static std::vector<OrOptCand> random_set(int n, int L, int max_far, bool few_gains)
{
    std::vector<OrOptCand> c;
    std::vector<char> used((size_t)L, 0);
    for (int i = 0; i < n; ++i) {
        const int k = 1 + (int)(rnd() % 3);
        if (L - 1 - k < 1) continue;
        const int a = 1 + (int)(rnd() % (uint64_t)(L - 1 - k)), h = a + k - 1;  // a >= 1, h <= L - 2
        const bool at_last = rnd() & 1;
        const int s = at_last ? h : a;
        if (used[s]) continue;
        const int far = 1 + (int)(rnd() % (uint64_t)max_far);
        int t = (rnd() & 1) ? h + far : a - 1 - far;
        if (t > L - 2) t = L - 2;
        if (t < 0) t = 0;
        if (t >= a - 1 && t <= h) continue;  // (clamped into the segment: no such move)
        used[s] = 1;
        const double g = few_gains ? 1.0 + (double)(rnd() % 3) : 1e-3 + (double)(rnd() % 1000003) / 7.0;
        c.push_back({g, s, a, t, or_opt_kr(k, k > 1 ? (int)(rnd() & 1) : 0)});
    }
    return c;
}

int main()
{
    // random sets: near and far insertions, distinct and repeated gains
    for (int rep = 0; rep < 600; ++rep) {
        const int L = 8 + (int)(rnd() % 400);
        one(random_set(1 + (int)(rnd() % 120), L, 1 + (int)(rnd() % 6), rep % 2), L);
        one(random_set(1 + (int)(rnd() % 120), L, L, rep % 3 == 0), L);
    }
    // nothing, one; the smallest paths, both fixed ends touched
    one({}, 100);
    one({cand(2.5, 1, 1, 2, 0)}, 4);
    one({cand(2.5, 2, 1, 0, 0)}, 4);
    one({cand(2.5, 1, 2, 3, 0)}, 5);
    one({cand(2.5, 2, 3, 0, 1)}, 6);
    one({cand(2.5, 1, 3, 4, 1, true)}, 6);
    one({cand(2.5, 3, 2, 97, 1)}, 100);
    // one move reported by both of its ends: accepted once
    one({cand(4.0, 10, 3, 50, 0), cand(4.0, 10, 3, 50, 0, true), cand(1.0, 60, 1, 62, 0)}, 100);
    // a forward and a backward move over the same range
    one({cand(4.0, 10, 2, 50, 0), cand(4.0, 49, 2, 9, 1, true)}, 100);
    one({cand(3.0, 10, 2, 50, 0), cand(4.0, 49, 2, 9, 1, true)}, 100);
    // all nested, best outermost / innermost / in the middle
    for (int mode = 0; mode < 3; ++mode) {
        std::vector<OrOptCand> c;
        for (int k = 0; k < 40; ++k) {
            const double g = mode == 0 ? 100.0 - k : (mode == 1 ? 1.0 + k : 50.0 - (k - 20) * (k - 20));
            c.push_back(cand(g + 1000.0, 1 + k, 1 + k % 3, 198 - k, 0));
        }
        one(c, 200);
    }
    // chains: ranges [lo, hi] then [hi, hi'] share edge hi, [lo, hi] then [hi+1, hi'] only touch
    for (int share = 0; share < 2; ++share)
        for (int order = 0; order < 3; ++order) {
            std::vector<OrOptCand> c;
            int at = 0;  // the next range's first edge
            for (int k = 0; k < 50; ++k) {
                const int seg = 1 + k % 3, len = seg + 1 + k % 4;
                const double g = order == 0 ? 1.0 + k : (order == 1 ? 100.0 - k : 1.0 + (k * 37) % 50);
                if (k % 2)
                    c.push_back(cand(g, at + 1, seg, at + len, 0));  // forward: [a-1, t]
                else
                    c.push_back(cand(g, at + len - seg + 1, seg, at, seg > 1, true));  // backward: [t, h]
                at += len + (share ? 0 : 1);
            }
            one(c, at + 2);
        }
    // equal gains everywhere: s ascending decides
    {
        std::vector<OrOptCand> c;
        for (int k = 0; k < 60; ++k) c.push_back(cand(3.0, 60 - k, 1 + k % 3, 60 - k + 3 + k % 5, 0));
        one(c, 200);
    }
    // max_seg below 3
    one({cand(2.0, 5, 1, 9, 0), cand(3.0, 20, 2, 30, 1)}, 100, 2);
    one({cand(2.0, 5, 1, 9, 0), cand(3.0, 20, 1, 3, 0)}, 100, 1);
    // refused inputs: nothing is accepted from them
    {
        int32_t lo[4], hi[4], how[4], pre[5];
        double gain = 0.0;
        OrOptCand good[2] = {cand(1.0, 1, 1, 2, 0), cand(1.0, 5, 3, 9, 1)};
        CHECK(or_opt_select(good, 2, 11, 3, lo, hi, how, pre, &gain) == 2);
        CHECK(or_opt_select(good, 2, 10, 3, lo, hi, how, pre, &gain) == -EINVAL);  // t > L - 2
        CHECK(or_opt_select(good, 2, 11, 2, lo, hi, how, pre, &gain) == -EINVAL);  // k > max_seg
        CHECK(or_opt_select(good, 2, 11, 0, lo, hi, how, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(good, 2, 11, 4, lo, hi, how, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(good, -1, 11, 3, lo, hi, how, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(nullptr, 2, 11, 3, lo, hi, how, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(good, 2, 11, 3, nullptr, hi, how, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(good, 2, 11, 3, lo, nullptr, how, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(good, 2, 11, 3, lo, hi, nullptr, pre, &gain) == -EINVAL);
        CHECK(or_opt_select(good, 2, 11, 3, lo, hi, how, nullptr, &gain) == -EINVAL);
        CHECK(or_opt_select(good, 2, 11, 3, lo, hi, how, pre, nullptr) == -EINVAL);
        CHECK(or_opt_select(nullptr, 0, 11, 3, nullptr, nullptr, nullptr, pre, &gain) == 0 && pre[0] == 0);
        cases += 13;
        const OrOptCand bad[] = {
            cand(-1.0, 3, 1, 6, 0),               // gain not > 0
            cand(0.0, 3, 1, 6, 0),                //
            cand(1.0, 0, 1, 6, 0),                // a < 1
            cand(1.0, 8, 3, 2, 0),                // h > L - 2
            cand(1.0, 3, 2, -1, 0),               // t < 0
            cand(1.0, 3, 2, 10, 0),               // t > L - 2
            cand(1.0, 3, 2, 2, 0),                // t = a - 1
            cand(1.0, 3, 2, 3, 0),                // t inside
            cand(1.0, 3, 2, 4, 0),                // t = h
            cand(1.0, 3, 1, 6, 1),                // k = 1 reversed
            {1.0, 3, 3, 6, 0},                    // k = 0
            {1.0, 3, 3, 6, 8 | 1},                // a bit above rev
            {1.0, 4, 3, 8, or_opt_kr(3, 0)},      // s inside the segment
            {1.0, 2, 3, 8, or_opt_kr(3, 0)},      // s outside it
        };
        for (const OrOptCand &b : bad) {
            OrOptCand one_bad[2] = {cand(5.0, 1, 1, 2, 0), b};
            CHECK(or_opt_select(one_bad, 2, 11, 3, lo, hi, how, pre, &gain) == -EINVAL);
            ++cases;
        }
        OrOptCand nan_gain[1] = {cand(__builtin_nan(""), 3, 1, 6, 0)};
        CHECK(or_opt_select(nan_gain, 1, 11, 3, lo, hi, how, pre, &gain) == -EINVAL);
        OrOptCand twice[2] = {cand(1.0, 3, 1, 5, 0), cand(1.0, 3, 2, 6, 0)};
        CHECK(or_opt_select(twice, 2, 11, 3, lo, hi, how, pre, &gain) == -EINVAL);
        cases += 2;
    }
    std::printf("check_or_opt: ok (%ld cases, %ld moves)\n", cases, moves_seen);
    return 0;
}
