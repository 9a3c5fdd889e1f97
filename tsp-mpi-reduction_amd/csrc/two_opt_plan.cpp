// see two_opt_plan.h
#include "two_opt_plan.h"

#include <algorithm>
#include <cerrno>
#include <iterator>
#include <map>

namespace tspgpu {

int two_opt_grid(int64_t L)
{
    int g = 1;
    while (g < kTwoOptMaxGrid && 2 * (int64_t)(g + 1) * (g + 1) <= L) ++g;
    return g;
}

int64_t two_opt_select(TwoOptCand *cand, int64_t n, int64_t L, int32_t *acc_i, int32_t *acc_j, int32_t *prefix,
                       double *gain)
{
    if (n < 0 || !prefix || !gain || (n > 0 && (!cand || !acc_i || !acc_j))) return -EINVAL;
    for (int64_t k = 0; k < n; ++k) {
        const TwoOptCand &c = cand[k];
        if (!(c.gain > 0.0) || c.i < 0 || c.j < (int64_t)c.i + 2 || c.j > L - 2) return -EINVAL;
    }
    std::sort(cand, cand + n, [](const TwoOptCand &a, const TwoOptCand &b) {
        return a.gain != b.gain ? a.gain > b.gain : a.i < b.i;
    });
    // the accepted ranges, disjoint: first edge -> last edge
    std::map<int32_t, int32_t> taken;
    int64_t m = 0;
    int32_t swaps = 0;
    prefix[0] = 0;
    for (int64_t k = 0; k < n; ++k) {
        const TwoOptCand &c = cand[k];
        if (k > 0 && cand[k - 1].gain == c.gain && cand[k - 1].i == c.i) return -EINVAL;
        const auto next = taken.upper_bound(c.i);  // the first range that starts behind i
        if (next != taken.end() && next->first <= c.j) continue;
        if (next != taken.begin() && std::prev(next)->second >= c.i) continue;
        taken.emplace_hint(next, c.i, c.j);
        acc_i[m] = c.i;
        acc_j[m] = c.j;
        swaps += (c.j - c.i) / 2;  // (disjoint ranges inside L <= 2^30 positions: below 2^29 in all)
        prefix[++m] = swaps;
        *gain = *gain + c.gain;
    }
    return m;
}

}  // namespace tspgpu
