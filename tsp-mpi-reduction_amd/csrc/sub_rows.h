// K1 variant 6 row table (hk_sub.h): one 16-byte entry per L-bit mask, built
// on the host (sub_rows.cpp, no HIP runtime needed) and decoded by sub_mid.
//
// Entry of a mask with J members:
//   nibbles 0..L-1  the members ascending, then the non-members ascending
//                   (L <= 10: ten nibbles, nibbles L..9 zero; L = 11: eleven)
//   from bit sub_row_field_bit0(L) (40 up to L = 10, 4 L above), for
//   2 <= J <= L-2, one field per non-member k_q (q = 0..L-J-1) for the
//   finished slot of destination row mask | (1 << k_q) in the next low layer,
//       (k_q - q) * C(L, J+1) + colex rank of that row
//   (k_q - q = position of k_q among the row's members; a layer is stored
//   position-major).  How the fields of a (L, J) are laid out is the first of
//   these that fits the 128 bits (sub_slot_mode):
//     0  the whole slot per field, sub_slot_bits wide, packed upwards, and a
//        field that would straddle a 32-bit word starts at the next word
//        instead — every (L, J) up to L = 10;
//     1  the whole slot, fields packed back to back (a field may straddle two
//        words: a two-word extract) — L = 11 at J = 2, 4, 5;
//     2  the colex rank only, laid out as in 0; the decoder adds
//        (k_q - q) * C(L, J+1) from the non-member's nibble — L = 11 at J = 3
//        (eight 11-bit slots are 88 bits, four more than the entry has left);
//     3  the colex rank only, packed as in 1 (no L so far).
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

constexpr int kSubRowMinL = 5, kSubRowMaxL = 11;
// first bit after the nibbles
TSPGPU_SUBROW_HD constexpr int sub_row_field_bit0(int L) { return L <= 10 ? 40 : 4 * L; }

TSPGPU_SUBROW_HD constexpr int sub_binom(int a, int b)
{
    if (b < 0 || b > a) return 0;
    int r = 1;
    for (int i = 1; i <= b; ++i) r = r * (a - b + i) / i;
    return r;
}
// values of the low layer J + 1 = one more than the largest slot
TSPGPU_SUBROW_HD constexpr int sub_slot_limit(int L, int J) { return sub_binom(L, J + 1) * (J + 1); }
// bits that hold every value below limit
TSPGPU_SUBROW_HD constexpr int sub_bits_for(int limit)
{
    int b = 1;
    while ((1 << b) < limit) ++b;
    return b;
}
// bit position of the q-th field of `bits` bits: packed back to back, or
// (aligned) moved to the next word where it would straddle one
TSPGPU_SUBROW_HD constexpr int sub_field_pos(int L, int bits, int q, bool packed)
{
    int pos = sub_row_field_bit0(L);
    if (packed) return pos + q * bits;
    for (int i = 0;; ++i) {
        if (pos / 32 != (pos + bits - 1) / 32) pos = (pos / 32 + 1) * 32;
        if (i == q) return pos;
        pos += bits;
    }
}
// field layout of an entry of J members (see the head of this file); -1: none fits
TSPGPU_SUBROW_HD constexpr int sub_slot_mode(int L, int J)
{
    const int nf = L - J;
    for (int mode = 0; mode < 4; ++mode) {
        const int bits = sub_bits_for(mode >= 2 ? sub_binom(L, J + 1) : sub_slot_limit(L, J));
        if (sub_field_pos(L, bits, nf - 1, (mode & 1) != 0) + bits <= 128) return mode;
    }
    return -1;
}
// whether a field holds the colex rank only (the decoder adds the position's layer offset)
TSPGPU_SUBROW_HD constexpr bool sub_slot_rank_only(int L, int J) { return sub_slot_mode(L, J) >= 2; }
TSPGPU_SUBROW_HD constexpr int sub_slot_bits(int L, int J)
{
    return sub_bits_for(sub_slot_rank_only(L, J) ? sub_binom(L, J + 1) : sub_slot_limit(L, J));
}
// bit position (0..127) of the q-th non-member's field in an entry of J members
TSPGPU_SUBROW_HD constexpr int sub_slot_pos(int L, int J, int q)
{
    return sub_field_pos(L, sub_slot_bits(L, J), q, (sub_slot_mode(L, J) & 1) != 0);
}
// whether an entry of J members carries slot fields (the middle passes' rows)
TSPGPU_SUBROW_HD constexpr bool sub_row_has_slots(int L, int J) { return J >= 2 && J <= L - 2; }
TSPGPU_SUBROW_HD constexpr bool sub_row_fits(int L)
{
    for (int J = 2; J <= L - 2; ++J)
        if (sub_slot_mode(L, J) < 0) return false;
    return true;
}
// every J of L in layout 0 (the only one there was up to L = 10)
TSPGPU_SUBROW_HD constexpr bool sub_row_plain(int L)
{
    for (int J = 2; J <= L - 2; ++J)
        if (sub_slot_mode(L, J) != 0) return false;
    return true;
}
static_assert(sub_row_fits(5) && sub_row_fits(6) && sub_row_fits(7) && sub_row_fits(8) && sub_row_fits(9) &&
                  sub_row_fits(10) && sub_row_fits(11),
              "slot fields fit the entry");
static_assert(sub_row_plain(5) && sub_row_plain(6) && sub_row_plain(7) && sub_row_plain(8) && sub_row_plain(9) &&
                  sub_row_plain(10),
              "L <= 10: whole slots, no field straddles a word");
static_assert(sub_slot_mode(11, 2) == 1 && sub_slot_mode(11, 3) == 2 && sub_slot_mode(11, 4) == 1 &&
                  sub_slot_mode(11, 5) == 1 && sub_slot_mode(11, 6) == 0 && sub_slot_mode(11, 7) == 0 &&
                  sub_slot_mode(11, 8) == 0 && sub_slot_mode(11, 9) == 0,
              "L = 11 layouts as documented");

// The table of L (kSubRowMinL..kSubRowMaxL) into rows, one entry per mask in
// (member count, value) order = TiledInfo::mask; false if L is out of range.
bool build_sub_rows(int L, std::vector<SubRow> &rows);

}  // namespace tspgpu
