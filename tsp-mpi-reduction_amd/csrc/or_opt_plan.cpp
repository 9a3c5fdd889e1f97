// see or_opt_plan.h
#include "or_opt_plan.h"

#include <algorithm>
#include <cerrno>
#include <iterator>
#include <map>

namespace tspgpu {

int64_t or_opt_select(OrOptCand *cand, int64_t n, int64_t L, int max_seg, int32_t *acc_lo, int32_t *acc_hi,
                      int32_t *acc_how, int32_t *prefix, double *gain)
{
    if (n < 0 || max_seg < 1 || max_seg > kOrOptMaxSeg || !prefix || !gain) return -EINVAL;
    if (n > 0 && (!cand || !acc_lo || !acc_hi || !acc_how)) return -EINVAL;
    for (int64_t m = 0; m < n; ++m) {
        const OrOptCand &c = cand[m];
        const int64_t k = c.kr & 3, a = c.a, h = a + k - 1, t = c.t;
        if (!(c.gain > 0.0) || (c.kr & ~7) || k < 1 || k > max_seg || (k == 1 && c.kr != 1)) return -EINVAL;
        if (a < 1 || h > L - 2 || t < 0 || t > L - 2 || (t >= a - 1 && t <= h)) return -EINVAL;
        if (c.s != a && c.s != h) return -EINVAL;
    }
    std::sort(cand, cand + n, [](const OrOptCand &x, const OrOptCand &y) {
        return x.gain != y.gain ? x.gain > y.gain : x.s < y.s;
    });
    // the accepted ranges, disjoint: first edge -> last edge
    std::map<int32_t, int32_t> taken;
    int64_t m = 0;
    int32_t total = 0;
    prefix[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const OrOptCand &c = cand[i];
        if (i > 0 && cand[i - 1].gain == c.gain && cand[i - 1].s == c.s) return -EINVAL;
        const int32_t k = c.kr & 3, h = c.a + k - 1;
        const bool fwd = c.t > h;
        const int32_t lo = fwd ? c.a - 1 : c.t, hi = fwd ? c.t : h;
        const auto next = taken.upper_bound(lo);  // the first range that starts behind lo
        if (next != taken.end() && next->first <= hi) continue;
        if (next != taken.begin() && std::prev(next)->second >= lo) continue;
        taken.emplace_hint(next, lo, hi);
        acc_lo[m] = lo;
        acc_hi[m] = hi;
        acc_how[m] = c.kr | (fwd ? kOrOptFwd : 0);
        total += hi - lo;  // (disjoint ranges inside L <= 2^30 positions: below 2^30 in all)
        prefix[++m] = total;
        *gain = *gain + c.gain;
    }
    return m;
}

}  // namespace tspgpu
