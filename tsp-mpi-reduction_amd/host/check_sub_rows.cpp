// K1 variant 6's row table (csrc/sub_rows.h, csrc/sub_rows.cpp) against its
// definition, for every L the builder accepts: host only, also built under
// ASan + UBSan (make check-sub-rows; tests/test_sub_rows.py).
//
// Per L: the entries are the masks in (member count, value) order; nibbles =
// members ascending, then non-members ascending; for 2 <= J <= L-2 the field of
// the q-th non-member k_q decodes to (k_q - q) * C(L, J+1) + colex rank of
// mask | (1 << k_q), which is below C(L, J+1) * (J+1); fields neither overlap
// each other or the nibbles nor cross a 32-bit word; every other bit is zero.
#include <cstdint>
#include <cstdio>
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
uint32_t get_bits(const SubRow &e, int pos, int bits)
{
    // (a field never crosses a word: checked before this is called)
    return (e.w[pos / 32] >> (pos % 32)) & (bits >= 32 ? ~0u : (1u << bits) - 1u);
}

long long check_L(int L)
{
    std::vector<SubRow> rows;
    if (!build_sub_rows(L, rows)) {
        fail(L, 0, "builder refused L");
        return 0;
    }
    if (rows.size() != (size_t)1 << L) fail(L, 0, "row count");
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
                const long long limit = pascal(L, J + 1) * (J + 1);
                if (sub_slot_limit(L, J) != limit || (1ll << bits) < limit) fail(L, m, "field width");
                for (int q = 0; q < (int)non.size(); ++q) {
                    const int pos = sub_slot_pos(L, J, q), k = non[q];
                    if (pos < kSubRowFieldBit0) fail(L, m, "field inside the nibbles");
                    if (pos / 32 != (pos + bits - 1) / 32 || pos + bits > 128) {
                        fail(L, m, "field crosses a word");
                        continue;
                    }
                    claim(pos, bits);
                    const long long want = (long long)(k - q) * pascal(L, J + 1) + colex_rank(m | (1u << k));
                    const uint32_t got = get_bits(e, pos, bits);
                    if ((long long)got != want) fail(L, m, "slot value");
                    if ((long long)got >= limit) fail(L, m, "slot not below the layer size");
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

}  // namespace

int main()
{
    std::vector<SubRow> rows;
    for (int L : {-1, 0, kSubRowMinL - 1, kSubRowMaxL + 1, 16, 31, 32})
        if (build_sub_rows(L, rows) || !rows.empty()) fail(L, 0, "builder accepted L");
    long long fields = 0;
    for (int L = kSubRowMinL; L <= kSubRowMaxL; ++L) fields += check_L(L);
    if (g_bad) {
        std::printf("check_sub_rows: %lld mismatches\n", g_bad);
        return 1;
    }
    std::printf("check_sub_rows: ok (L = %d..%d, %lld slot fields)\n", kSubRowMinL, kSubRowMaxL, fields);
    return 0;
}
