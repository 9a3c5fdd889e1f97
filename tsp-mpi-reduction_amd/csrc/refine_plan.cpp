// Host plan of the window refinement: see refine_plan.h.
#include "refine_plan.h"

#include <cerrno>
#include <climits>

namespace tspgpu {

int refine_pass(int64_t L, int m, int pass, int strict, RefinePass *out)
{
    if (!out || L < 2 || pass < 0) return -EINVAL;
    if (m < kRefineMinM || m > (strict ? kRefineStrictMaxM : kRefineMaxM)) return -EINVAL;
    RefinePass p;
    p.stride = m + 1;
    p.w = m + 2;
    p.offset = (pass & 1) ? (m + 1) / 2 : 0;
    // window k covers offset + k*stride .. offset + k*stride + m + 1 <= L - 1
    const int64_t room = L - 1 - p.offset;
    p.windows = room > 0 ? room / p.stride : 0;
    if (p.windows > INT_MAX) return -EINVAL;
    p.cities = p.windows * p.w;
    p.dist = p.cities * p.w;
    p.fold = p.windows * (int64_t)(p.w - 1) * (p.w - 1);
    *out = p;
    return 0;
}

bool refine_stop(int pass, int max_passes, int64_t replaced, int64_t replaced_before)
{
    if (pass + 1 >= max_passes) return true;
    return pass >= 1 && replaced == 0 && replaced_before == 0;
}

}  // namespace tspgpu
