// K1 variant 6's row table (csrc/sub_rows.h, csrc/sub_rows.cpp) against its
// definition, for every L the builder accepts: host only, also built under
// ASan + UBSan (make check-sub-rows; tests/test_sub_rows.py).
//
// Per L: the entries are the masks in (member count, value) order; nibbles =
// members ascending, then non-members ascending; for 2 <= J <= L-2 the field of
// the q-th non-member k_q decodes to (k_q - q) * C(L, J+1) + colex rank of
// mask | (1 << k_q), which is below C(L, J+1) * (J+1) — or, where the header
// says the (L, J) keeps the rank only, to that rank, below C(L, J+1); fields
// neither overlap each other or the nibbles nor leave the entry; every other
// bit is zero.  Up to L = 10 the layout is also compared with the original
// rule written out here on its own (whole slots from bit 40, no field crossing
// a 32-bit word), so those tables keep their bits; at L = 11 a field may cross
// a word where the header says so, and is then read from both words.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sub_rows.h"

using namespace tspgpu;

namespace {

long long g_bad = 0;
void fail(int L, uint32_t m, const char *what)
{
    if (g_bad++ < 20) std::printf("L=%d mask=0x%x: %s\n", L, m, what);
}

// independent of the builder: Pascal's triangle, and the colex rank as the
// sum over the members e_i ascending (i = 1..) of C(e_i, i)
long long pascal(int a, int b)
{
    static long long t[16][16];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) t[i][j] = j == 0 ? 1 : (i == 0 ? 0 : t[i - 1][j - 1] + t[i - 1][j]);
        init = true;
    }
    return b < 0 || b > a ? 0 : t[a][b];
}
long long colex_rank(uint32_t m)
{
    long long r = 0;
    int i = 0;
    for (int b = 0; b < 16; ++b)
        if (m >> b & 1) r += pascal(b, ++i);
    return r;
}
// bits pos..pos+bits-1 of the 128-bit entry (inside it: checked before this is called)
uint32_t get_bits(const SubRow &e, int pos, int bits)
{
    uint64_t v = e.w[pos / 32];
    if (pos / 32 + 1 < 4) v |= (uint64_t)e.w[pos / 32 + 1] << 32;
    return (uint32_t)(v >> (pos % 32)) & (bits >= 32 ? ~0u : (1u << bits) - 1u);
}
// the original layout (L <= 10): fields of the whole slot's width from bit 40,
// a field that would cross a word moved to the next one
int legacy_pos(int bits, int q)
{
    int pos = 40;
    for (int i = 0;; ++i) {
        if (pos / 32 != (pos + bits - 1) / 32) pos = (pos / 32 + 1) * 32;
        if (i == q) return pos;
        pos += bits;
    }
}

long long check_L(int L)
{
    std::vector<SubRow> rows;
    if (!build_sub_rows(L, rows)) {
        fail(L, 0, "builder refused L");
        return 0;
    }
    if (rows.size() != (size_t)1 << L) fail(L, 0, "row count");
    if (sub_row_field_bit0(L) < 4 * L) fail(L, 0, "fields start inside the nibbles");
    long long fields = 0;
    size_t idx = 0;
    for (int J = 0; J <= L; ++J)
        for (uint32_t m = 0; m < (1u << L); ++m) {
            if (__builtin_popcount(m) != J) continue;
            if (idx >= rows.size()) return fields;
            const SubRow &e = rows[idx++];
            uint32_t used[4] = {0, 0, 0, 0};
            auto claim = [&](int pos, int bits) {
                for (int b = pos; b < pos + bits; ++b) {
                    if (b < 0 || b >= 128) {
                        fail(L, m, "field outside the entry");
                        return;
                    }
                    if (used[b / 32] >> (b % 32) & 1) fail(L, m, "fields overlap");
                    used[b / 32] |= 1u << (b % 32);
                }
            };
            // nibbles: members, then non-members, ascending
            int nib = 0;
            std::vector<int> non;
            for (int b = 0; b < L; ++b)
                if (m >> b & 1) {
                    if (get_bits(e, 4 * nib, 4) != (uint32_t)b) fail(L, m, "member nibble");
                    ++nib;
                }
            for (int b = 0; b < L; ++b)
                if (!(m >> b & 1)) {
                    if (get_bits(e, 4 * nib, 4) != (uint32_t)b) fail(L, m, "non-member nibble");
                    ++nib;
                    non.push_back(b);
                }
            claim(0, 4 * L);
            if (J >= 2 && J <= L - 2) {
                if (!sub_row_has_slots(L, J)) fail(L, m, "sub_row_has_slots");
                const int bits = sub_slot_bits(L, J);
                const bool rank_only = sub_slot_rank_only(L, J);
                const long long limit = rank_only ? pascal(L, J + 1) : pascal(L, J + 1) * (J + 1);
                if (sub_slot_limit(L, J) != pascal(L, J + 1) * (J + 1) || (1ll << bits) < limit)
                    fail(L, m, "field width");
                if (L <= 10 && (rank_only || (1ll << (bits - 1)) >= limit)) fail(L, m, "L <= 10: whole slots, tight width");
                for (int q = 0; q < (int)non.size(); ++q) {
                    const int pos = sub_slot_pos(L, J, q), k = non[q];
                    if (pos < sub_row_field_bit0(L)) fail(L, m, "field inside the nibbles");
                    if (L <= 10 && (pos != legacy_pos(bits, q) || pos / 32 != (pos + bits - 1) / 32))
                        fail(L, m, "L <= 10: not the original layout");
                    if (pos + bits > 128) {
                        fail(L, m, "field outside the entry");
                        continue;
                    }
                    claim(pos, bits);
                    const long long want =
                        (rank_only ? 0 : (long long)(k - q) * pascal(L, J + 1)) + colex_rank(m | (1u << k));
                    const uint32_t got = get_bits(e, pos, bits);
                    if ((long long)got != want) fail(L, m, "slot value");
                    if ((long long)got >= limit) fail(L, m, "slot not below the layer size");
                    // what the decoder stores to: the field, plus the position's offset where it keeps the rank only
                    const long long slot = got + (rank_only ? (long long)(k - q) * pascal(L, J + 1) : 0);
                    if (slot < 0 || slot >= pascal(L, J + 1) * (J + 1)) fail(L, m, "decoded slot outside the layer");
                    ++fields;
                }
            } else if (sub_row_has_slots(L, J)) {
                fail(L, m, "sub_row_has_slots outside the middle passes");
            }
            for (int w = 0; w < 4; ++w)
                if (e.w[w] & ~used[w]) fail(L, m, "unused bit set");
        }
    return fields;
}

// --dump L: the layout the header gives every J of L ("layout J rank_only bits
// pos_0 .. pos_(L-J-1)") and the table as built ("entry w0 w1 w2 w3", in table
// order), for a decoder outside this program (tests/test_sub_rows_l11.py)
int dump(int L)
{
    std::vector<SubRow> rows;
    if (!build_sub_rows(L, rows)) return 1;
    std::printf("field_bit0 %d\n", sub_row_field_bit0(L));
    for (int J = 2; J <= L - 2; ++J) {
        std::printf("layout %d %d %d", J, sub_slot_rank_only(L, J) ? 1 : 0, sub_slot_bits(L, J));
        for (int q = 0; q < L - J; ++q) std::printf(" %d", sub_slot_pos(L, J, q));
        std::printf("\n");
    }
    for (const SubRow &e : rows) std::printf("entry %08x %08x %08x %08x\n", e.w[0], e.w[1], e.w[2], e.w[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "--dump") return dump(std::atoi(argv[2]));
    std::vector<SubRow> rows;
    for (int L : {-1, 0, kSubRowMinL - 1, kSubRowMaxL + 1, 16, 31, 32})
        if (build_sub_rows(L, rows) || !rows.empty()) fail(L, 0, "builder accepted L");
    // the sizes whose tables must keep their bits, then L = 11 (its own line)
    long long fields = 0, fields11 = 0;
    for (int L = kSubRowMinL; L <= 10; ++L) fields += check_L(L);
    static_assert(kSubRowMaxL == 11, "a larger L wants its own line");
    fields11 = check_L(11);
    if (g_bad) {
        std::printf("check_sub_rows: %lld mismatches\n", g_bad);
        return 1;
    }
    std::printf("check_sub_rows: ok (L = %d..%d, %lld slot fields)\n", kSubRowMinL, 10, fields);
    std::printf("check_sub_rows: ok (L = 11, %lld slot fields)\n", fields11);
    return 0;
}
