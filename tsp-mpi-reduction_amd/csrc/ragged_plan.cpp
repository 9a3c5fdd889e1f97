// Host plan of a ragged K1 batch (ragged_plan.h): a stable counting sort of
// the blocks by city count and the staging layout of the buckets.
#include "ragged_plan.h"

#include <cerrno>
#include <climits>

namespace tspgpu {

namespace {

// next multiple of 256 bytes, in elements of `bytes` bytes (256 % bytes == 0)
int64_t align_elems(int64_t elems, int bytes)
{
    const int64_t q = (int64_t)kRaggedAlignBytes / bytes;
    return (elems + q - 1) / q * q;
}

}  // namespace

int ragged_plan(const int32_t *n, const int64_t *offset, int nblocks, int strict, int vbytes, RaggedPlan *plan)
{
    if (!plan || nblocks < 0 || (vbytes != 8 && vbytes != 4)) return -EINVAL;
    if (nblocks > 0 && (!n || !offset)) return -EINVAL;
    *plan = RaggedPlan();
    plan->nblocks = nblocks;
    plan->pre.assign((size_t)nblocks, 0);
    plan->slot.assign((size_t)nblocks, -1);
    plan->desc.assign((size_t)nblocks, RaggedDesc{0, 0, 0, 0, 0, 0});
    const int max_n = strict ? kRaggedStrictMaxN : kRaggedMaxN;
    constexpr int64_t kMaxElems = (int64_t)kRaggedMaxN * kRaggedMaxN;

    // refuse, count
    for (int b = 0; b < nblocks; ++b) {
        // (an offset whose matrix would end past INT64_MAX is refused like a negative one)
        if (n[b] < kRaggedMinN || n[b] > max_n || offset[b] < 0 || offset[b] > INT64_MAX - kMaxElems) {
            plan->pre[b] = -EINVAL;
            plan->desc[b].pre = (int16_t)-EINVAL;
            continue;
        }
        const int64_t lo = offset[b], hi = offset[b] + (int64_t)n[b] * n[b];
        if (plan->in_range == 0 || lo < plan->ext_lo) plan->ext_lo = lo;
        if (plan->in_range == 0 || hi > plan->ext_hi) plan->ext_hi = hi;
        if (n[b] > plan->max_n) plan->max_n = n[b];
        ++plan->count[n[b]];
        ++plan->in_range;
    }

    // bucket ranges and staging bases
    int at = 0;
    int64_t d = 0, c = 0, t = 0;
    for (int k = kRaggedMinN; k <= kRaggedMaxN; ++k) {
        plan->begin[k] = at;
        at += plan->count[k];
        plan->dist_base[k] = d;
        plan->cost_base[k] = c;
        plan->tour_base[k] = t;
        d = align_elems(d + (int64_t)plan->count[k] * k * k, vbytes);
        c = align_elems(c + plan->count[k], vbytes);
        t = align_elems(t + (int64_t)plan->count[k] * (k + 1), 4);
    }
    plan->dist_elems = d;
    plan->cost_elems = c;
    plan->tour_elems = t;
    if (c > INT32_MAX) return -EINVAL;  // (RaggedDesc::cost; nblocks <= INT_MAX leaves room for the padding)

    // stable placement: caller order inside every bucket
    plan->order.assign((size_t)plan->in_range, 0);
    int fill[kRaggedMaxN + 1] = {};
    for (int b = 0; b < nblocks; ++b) {
        if (plan->pre[b]) continue;
        const int k = n[b], s = fill[k]++;
        plan->slot[b] = s;
        plan->order[(size_t)plan->begin[k] + s] = b;
        RaggedDesc &e = plan->desc[b];
        e.src = offset[b];
        e.dst = plan->dist_base[k] + (int64_t)s * k * k;
        e.tour = plan->tour_base[k] + (int64_t)s * (k + 1);
        e.cost = (int32_t)(plan->cost_base[k] + s);
        e.n = (int16_t)k;
        e.pre = 0;
    }
    return 0;
}

}  // namespace tspgpu
