// K1 variant 6 row table (hk_sub.h): one 16-byte entry per L-bit mask, built
// on the host (sub_rows.cpp, no HIP runtime needed) and decoded by sub_mid.
//
// Entry of a mask with J members, L <= 10:
//   bits 0..39   nibbles 0..L-1: the members ascending, then the non-members
//                ascending (nibbles L..9 zero)
//   from bit 40  for 2 <= J <= L-2, one field per non-member k_q (q = 0..L-J-1):
//                the finished slot of destination row mask | (1 << k_q) in the
//                next low layer, (k_q - q) * C(L, J+1) + colex rank of that row
//                (k_q - q = position of k_q among the row's members; a layer is
//                stored position-major).  Fields are sub_slot_bits(L, J) wide,
//                packed upwards, and a field that would straddle a 32-bit word
//                starts at the next word instead.
// Every other bit is zero.  The layout functions below are the only
// description of it: the builder and the kernel both call them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSPGPU_SUBROW_HD __host__ __device__
#else
#define TSPGPU_SUBROW_HD
#endif

namespace tspgpu {

struct SubRow {
    uint32_t w[4];
};

constexpr int kSubRowMinL = 5, kSubRowMaxL = 10;
constexpr int kSubRowFieldBit0 = 40;  // first bit after the ten nibbles

TSPGPU_SUBROW_HD constexpr int sub_binom(int a, int b)
{
    if (b < 0 || b > a) return 0;
    int r = 1;
    for (int i = 1; i <= b; ++i) r = r * (a - b + i) / i;
    return r;
}
// values of the low layer J + 1 = one more than the largest slot
TSPGPU_SUBROW_HD constexpr int sub_slot_limit(int L, int J) { return sub_binom(L, J + 1) * (J + 1); }
TSPGPU_SUBROW_HD constexpr int sub_slot_bits(int L, int J)
{
    int b = 1;
    while ((1 << b) < sub_slot_limit(L, J)) ++b;
    return b;
}
// bit position (0..127) of the q-th non-member's field in an entry of J members
TSPGPU_SUBROW_HD constexpr int sub_slot_pos(int L, int J, int q)
{
    const int bits = sub_slot_bits(L, J);
    int pos = kSubRowFieldBit0;
    for (int i = 0;; ++i) {
        if (pos / 32 != (pos + bits - 1) / 32) pos = (pos / 32 + 1) * 32;
        if (i == q) return pos;
        pos += bits;
    }
}
// whether an entry of J members carries slot fields (the middle passes' rows)
TSPGPU_SUBROW_HD constexpr bool sub_row_has_slots(int L, int J) { return J >= 2 && J <= L - 2; }
TSPGPU_SUBROW_HD constexpr bool sub_row_fits(int L)
{
    for (int J = 2; J <= L - 2; ++J)
        if (sub_slot_pos(L, J, L - J - 1) + sub_slot_bits(L, J) > 128) return false;
    return true;
}
static_assert(sub_row_fits(5) && sub_row_fits(6) && sub_row_fits(7) && sub_row_fits(8) && sub_row_fits(9) &&
                  sub_row_fits(10),
              "slot fields fit the entry");

// The table of L (kSubRowMinL..kSubRowMaxL) into rows, one entry per mask in
// (member count, value) order = TiledInfo::mask; false if L is out of range.
bool build_sub_rows(int L, std::vector<SubRow> &rows);

}  // namespace tspgpu
