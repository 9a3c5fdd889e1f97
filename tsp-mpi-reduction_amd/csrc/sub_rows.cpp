// Host builder of K1 variant 6's row table (sub_rows.h): plain C++, no HIP.
#include "sub_rows.h"

namespace tspgpu {

bool build_sub_rows(int L, std::vector<SubRow> &rows)
{
    rows.clear();
    if (L < kSubRowMinL || L > kSubRowMaxL) return false;
    std::vector<int> rank((size_t)1 << L, 0);
    std::vector<uint32_t> order;  // masks by (popcount, value); numeric order of equal-popcount masks = colex order
    order.reserve((size_t)1 << L);
    for (int j = 0; j <= L; ++j) {
        int r = 0;
        for (uint32_t m = 0; m < (1u << L); ++m)
            if (__builtin_popcount(m) == j) {
                rank[m] = r++;
                order.push_back(m);
            }
    }
    rows.resize(order.size());
    for (size_t i = 0; i < order.size(); ++i) {
        const uint32_t m = order[i];
        const int J = __builtin_popcount(m);
        SubRow e = {{0u, 0u, 0u, 0u}};
        // (a field that straddles two words, layouts 1 and 3: its high bits go to the next word)
        auto put = [&](int pos, uint32_t v) {
            e.w[pos / 32] |= v << (pos % 32);
            if (pos % 32 && (v >> (32 - pos % 32))) e.w[pos / 32 + 1] |= v >> (32 - pos % 32);
        };
        int nib = 0;
        for (int b = 0; b < L; ++b)
            if (m >> b & 1) put(4 * nib++, (uint32_t)b);
        int q = 0;
        for (int b = 0; b < L; ++b)
            if (!(m >> b & 1)) {
                put(4 * nib++, (uint32_t)b);
                if (sub_row_has_slots(L, J)) {
                    const int layer_off = sub_slot_rank_only(L, J) ? 0 : (b - q) * sub_binom(L, J + 1);
                    put(sub_slot_pos(L, J, q), (uint32_t)(layer_off + rank[m | (1u << b)]));
                }
                ++q;
            }
        rows[i] = e;
    }
    return true;
}

}  // namespace tspgpu
