// The ragged batch plan (csrc/ragged_plan.h, csrc/ragged_plan.cpp) against its
// definition: host only, also built under ASan + UBSan (make check-ragged;
// tests/test_ragged_plan.py).
//
// Expectations are computed here, not with the planner: the in-range blocks
// through std::stable_sort of their indices by n, the bucket positions and the
// staging sizes through running sums.  Checked per case: refused blocks carry
// -EINVAL, slot -1 and a zero descriptor and are in no bucket; the order is the
// stable sort's; slots are a bijection onto the bucket positions, in caller
// order; bucket bases are multiples of 256 bytes and no two buckets (nor two
// blocks) overlap in any of the three staging areas; extent and largest n.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ragged_plan.h"

using namespace tspgpu;

namespace {

long long g_bad = 0, g_cases = 0, g_blocks = 0;
void fail(const std::string &name, const char *what, long long at = -1)
{
    if (g_bad++ < 20) std::printf("%s: %s (%lld)\n", name.c_str(), what, at);
}

struct Span {
    int64_t lo, hi;
};
// no two spans overlap (empty spans are dropped)
bool disjoint(std::vector<Span> v)
{
    v.erase(std::remove_if(v.begin(), v.end(), [](const Span &s) { return s.hi <= s.lo; }), v.end());
    std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i].lo < v[i - 1].hi) return false;
    return true;
}

void check(const std::string &name, const std::vector<int32_t> &n, const std::vector<int64_t> &off, int strict,
           int vbytes)
{
    ++g_cases;
    const int B = (int)n.size();
    g_blocks += B;
    RaggedPlan p;
    const int rc = ragged_plan(n.data(), off.data(), B, strict, vbytes, &p);
    if (rc) return fail(name, "planner returned an error", rc);

    const int cap = strict ? 16 : 20;
    std::vector<int> good;
    int want_max = 0;
    int64_t lo = 0, hi = 0;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 2 || n[b] > cap || off[b] < 0) continue;
        const int64_t e = off[b] + (int64_t)n[b] * n[b];
        if (good.empty() || off[b] < lo) lo = off[b];
        if (good.empty() || e > hi) hi = e;
        want_max = std::max(want_max, (int)n[b]);
        good.push_back(b);
    }
    std::stable_sort(good.begin(), good.end(), [&](int a, int b) { return n[a] < n[b]; });

    if (p.nblocks != B || (int)p.pre.size() != B || (int)p.slot.size() != B || (int)p.desc.size() != B)
        return fail(name, "table sizes");
    if (p.in_range != (int)good.size() || p.order.size() != good.size()) return fail(name, "in-range count");
    if (p.max_n != want_max) fail(name, "largest n", p.max_n);
    if (p.ext_lo != lo || p.ext_hi != hi) fail(name, "covering extent");
    for (size_t i = 0; i < good.size(); ++i)
        if (p.order[i] != good[i]) {
            fail(name, "order is not the stable sort by n", (long long)i);
            break;
        }

    // refused blocks
    std::vector<char> is_good((size_t)B, 0);
    for (int b : good) is_good[b] = 1;
    for (int b = 0; b < B; ++b) {
        const RaggedDesc &e = p.desc[b];
        if (is_good[b]) {
            if (p.pre[b] != 0 || e.pre != 0) fail(name, "in-range block refused", b);
            continue;
        }
        if (p.pre[b] != -EINVAL || e.pre != -EINVAL) fail(name, "refused block without -EINVAL", b);
        if (p.slot[b] != -1 || e.n != 0 || e.src != 0 || e.dst != 0 || e.tour != 0 || e.cost != 0)
            fail(name, "refused block has a slot", b);
    }

    // buckets: ranges by running sums, slots a bijection in caller order
    const int64_t q = 256 / vbytes;
    int at = 0, total = 0;
    std::vector<Span> dspan, cspan, tspan, dblk, tblk;
    std::vector<int64_t> cidx;
    for (int k = 0; k <= 20; ++k) {
        int cnt = 0;
        for (int b : good) cnt += n[b] == k;
        if (k < 2) {
            if (p.count[k] != 0) fail(name, "bucket below 2 cities", k);
            continue;
        }
        if (p.count[k] != cnt || p.begin[k] != at) fail(name, "bucket range", k);
        if (p.dist_base[k] % q || p.cost_base[k] % q || p.tour_base[k] % 64) fail(name, "bucket base not 256-byte aligned", k);
        if (p.dist_base[k] < 0 || p.cost_base[k] < 0 || p.tour_base[k] < 0) fail(name, "negative base", k);
        dspan.push_back({p.dist_base[k], p.dist_base[k] + (int64_t)cnt * k * k});
        cspan.push_back({p.cost_base[k], p.cost_base[k] + cnt});
        tspan.push_back({p.tour_base[k], p.tour_base[k] + (int64_t)cnt * (k + 1)});
        if (dspan.back().hi > p.dist_elems || cspan.back().hi > p.cost_elems || tspan.back().hi > p.tour_elems)
            fail(name, "bucket beyond the staging size", k);
        int s = 0, prev = -1;
        for (int i = at; i < at + cnt && i < (int)p.order.size(); ++i, ++s) {
            const int b = p.order[i];
            const RaggedDesc &e = p.desc[b];
            if (b <= prev) fail(name, "bucket not in caller order", b);
            prev = b;
            if (p.slot[b] != s) fail(name, "slot", b);
            if (e.n != k || e.src != off[b]) fail(name, "descriptor n / source", b);
            if (e.dst != p.dist_base[k] + (int64_t)s * k * k) fail(name, "descriptor destination", b);
            if (e.tour != p.tour_base[k] + (int64_t)s * (k + 1)) fail(name, "descriptor tour", b);
            if (e.cost != p.cost_base[k] + s) fail(name, "descriptor cost", b);
            dblk.push_back({e.dst, e.dst + (int64_t)k * k});
            tblk.push_back({e.tour, e.tour + k + 1});
            cidx.push_back(e.cost);
        }
        at += cnt;
        total += cnt;
    }
    if (total != (int)good.size()) fail(name, "buckets do not hold every in-range block");
    if (!disjoint(dspan) || !disjoint(cspan) || !disjoint(tspan)) fail(name, "buckets overlap");
    if (!disjoint(dblk) || !disjoint(tblk)) fail(name, "block slots overlap");
    std::sort(cidx.begin(), cidx.end());
    if (std::adjacent_find(cidx.begin(), cidx.end()) != cidx.end()) fail(name, "two blocks share a cost index");
}

// packed offsets in caller order
std::vector<int64_t> packed(const std::vector<int32_t> &n)
{
    std::vector<int64_t> off;
    int64_t at = 0;
    for (int32_t k : n) {
        off.push_back(at);
        at += k > 0 ? (int64_t)k * k : 0;
    }
    return off;
}

}  // namespace

int main()
{
    std::mt19937 rng(20260);
    for (int vbytes : {8, 4})
        for (int strict : {0, 1}) {
            const std::string tag = std::string(vbytes == 8 ? " f64" : " i32") + (strict ? " strict" : "");
            check("empty" + tag, {}, {}, strict, vbytes);
            check("one block" + tag, {7}, {0}, strict, vbytes);
            check("one refused block" + tag, {21}, {0}, strict, vbytes);
            {
                std::vector<int32_t> n(37, 9);
                check("one size" + tag, n, packed(n), strict, vbytes);
            }
            {
                std::vector<int32_t> n;
                for (int r = 0; r < 3; ++r)
                    for (int k = 20; k >= 2; --k) n.push_back(k);  // (17..20 refused under strict)
                check("every size" + tag, n, packed(n), strict, vbytes);
            }
            {
                std::vector<int32_t> n(1000);
                for (auto &k : n) k = 2 + (int)(rng() % 19);
                check("1000 random" + tag, n, packed(n), strict, vbytes);
            }
            {
                // sizes 5 and 7 with none of 6; 12 and 16 with nothing between
                std::vector<int32_t> n = {7, 5, 16, 5, 12, 7, 7, 16, 5};
                check("empty size between" + tag, n, packed(n), strict, vbytes);
            }
            {
                std::vector<int32_t> n = {8, -3, 0, 9, 1, 21, 17, 8, 16, INT32_MIN, INT32_MAX};
                check("bad n" + tag, n, packed(n), strict, vbytes);
            }
            {
                std::vector<int32_t> n = {6, 6, 10, 6};
                check("negative offset" + tag, n, {100, -1, 0, INT64_MIN}, strict, vbytes);
                // the covering extent ignores refused blocks
                check("refused outside" + tag, {5, 21, 5, 3}, {1000, 5, 2000, -7}, strict, vbytes);
            }
            {
                std::vector<int32_t> n = {4, 4, 9, 4, 9, 13};
                check("repeated offsets" + tag, n, {50, 50, 50, 50, 0, 0}, strict, vbytes);
                check("descending offsets" + tag, n, {900, 700, 500, 300, 100, 0}, strict, vbytes);
                check("overlapping offsets" + tag, n, {0, 3, 5, 7, 11, 1}, strict, vbytes);
                check("odd gaps" + tag, n, {1, 18, 35, 117, 134, 216}, strict, vbytes);
            }
            {
                std::vector<int32_t> n(1000);
                std::vector<int64_t> off(1000);
                for (int b = 0; b < 1000; ++b) {
                    n[b] = (int)(rng() % 26) - 2;  // -2..23: some refused
                    off[b] = (int64_t)(rng() % 5000) - 50;
                }
                check("1000 random with refusals" + tag, n, off, strict, vbytes);
            }
        }

    // call-level refusals
    RaggedPlan p;
    const int32_t n1[1] = {5};
    const int64_t o1[1] = {0};
    if (ragged_plan(n1, o1, -1, 0, 8, &p) != -EINVAL) fail("call", "nblocks < 0 accepted");
    if (ragged_plan(nullptr, o1, 1, 0, 8, &p) != -EINVAL) fail("call", "NULL n accepted");
    if (ragged_plan(n1, nullptr, 1, 0, 8, &p) != -EINVAL) fail("call", "NULL offset accepted");
    if (ragged_plan(n1, o1, 1, 0, 2, &p) != -EINVAL) fail("call", "value size 2 accepted");
    if (ragged_plan(n1, o1, 1, 0, 8, nullptr) != -EINVAL) fail("call", "NULL plan accepted");
    if (ragged_plan(nullptr, nullptr, 0, 0, 4, &p) != 0) fail("call", "empty batch with NULL arrays refused");
    // an offset whose matrix would end past INT64_MAX is refused, not overflowed
    const int64_t o2[1] = {INT64_MAX - 10};
    if (ragged_plan(n1, o2, 1, 0, 8, &p) != 0 || p.pre[0] != -EINVAL || p.in_range != 0)
        fail("call", "offset near INT64_MAX");

    if (g_bad) {
        std::printf("check_ragged: %lld mismatches\n", g_bad);
        return 1;
    }
    std::printf("check_ragged: ok (%lld cases, %lld blocks)\n", g_cases, g_blocks);
    return 0;
}
