// The exactness rules of the device distance build (csrc/dist_exact.h) as host
// code against glibc (make check-dist-exact; tests/test_dist_exact.py), plain
// and under ASan + UBSan.
//
//  - unflagged by square_needs_host  =>  pow(dx, 2) has the bits of dx*dx
//  - pow(-dx, 2) has the bits of pow(dx, 2) (the device stores one square per
//    unordered pair)
//  - sqrt_rn(a) has the bits of sqrt(a), and its acceptance test takes sqrt(a)
//    and refuses both neighbours
//  - the generator-style sample holds at least 1000 values with
//    pow(dx, 2) != dx*dx (else the first check would see nothing) and flags
//    fewer than 12% (else "flag everything" would pass)
// pow and sqrt are called through volatile pointers (-fno-builtin-pow), as
// tspgpu_distance_matrix calls them.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dist_exact.h"

namespace {

double (*volatile pow_fn)(double, double) = ::pow;
double (*volatile sqrt_fn)(double) = ::sqrt;

using tspgpu::dist_bits;

long long g_fail = 0;

void fail(const char *what, double a, double got, double want)
{
    if (++g_fail <= 20)
        std::fprintf(stderr, "check_dist_exact: %s: input %a: got %a, want %a\n", what, a, got, want);
}

struct Tally {
    long long values = 0, flagged = 0, differ = 0;
};

// the two square rules on one difference
void check_square(double dx, Tally *t)
{
    double p;
    const bool flag = tspgpu::square_needs_host(dx, &p);
    const double pw = pow_fn(dx, 2);
    ++t->values;
    if (flag) ++t->flagged;
    if (std::isnan(pw)) {
        if (!flag) fail("NaN square not flagged", dx, p, pw);
        return;
    }
    if (dist_bits(pw) != dist_bits(p)) {
        ++t->differ;
        if (!flag) fail("unflagged but pow(dx,2) != dx*dx", dx, p, pw);
    }
    const double pn = pow_fn(-dx, 2);
    if (dist_bits(pn) != dist_bits(pw)) fail("pow(-dx,2) != pow(dx,2)", dx, pn, pw);
}

long long g_sqrt = 0;

void check_sqrt(double a)
{
    ++g_sqrt;
    const double want = sqrt_fn(a), got = tspgpu::sqrt_rn(a);
    if (std::isnan(want)) {
        if (!std::isnan(got)) fail("sqrt_rn of NaN", a, got, want);
        return;
    }
    if (dist_bits(got) != dist_bits(want)) fail("sqrt_rn(a) != sqrt(a)", a, got, want);
    // the acceptance test itself: glibc's root and never a neighbour
    if (a >= 0x1p-900 && a <= DBL_MAX) {
        if (!tspgpu::sqrt_rn_accepts(want, a)) fail("sqrt(a) not accepted", a, want, want);
        const double lo = std::nextafter(want, 0.0), hi = std::nextafter(want, INFINITY);
        if (tspgpu::sqrt_rn_accepts(lo, a)) fail("lower neighbour accepted", a, lo, want);
        if (std::isfinite(hi) && tspgpu::sqrt_rn_accepts(hi, a)) fail("upper neighbour accepted", a, hi, want);
    }
}

double frand() { return (double)std::rand() / RAND_MAX; }

}  // namespace

int main()
{
    // (1) differences of coordinates drawn the way tsphost_generate_grid draws
    // them: float block extents, lo + rand()/RAND_MAX * (hi - lo), all pairs of
    // a block's 16 cities, x and y
    Tally gen;
    std::vector<double> sums;  // pow(dx,2) + pow(dy,2) of every 3rd pair, for sqrt_rn
    const int kN = 16;
    const struct {
        int grid, R;
    } cfg[] = {{1000, 1}, {1000, 256}, {8000, 16}, {1000, 4}};
    for (const auto &g : cfg) {
        const float span = g.grid / (float)g.R;
        for (int b = 0; b < 11000; ++b) {
            const int row = b % g.R, col = (b / 7) % g.R;
            const float x_lo = row * span, x_hi = (row + 1) * span;
            const float y_lo = col * span, y_hi = (col + 1) * span;
            double x[kN], y[kN];
            for (int j = 0; j < kN; ++j) {
                x[j] = (double)x_lo + frand() * ((double)x_hi - (double)x_lo);
                y[j] = (double)y_lo + frand() * ((double)y_hi - (double)y_lo);
            }
            for (int i = 0; i < kN; ++i)
                for (int j = i + 1; j < kN; ++j) {
                    const double dx = x[i] - x[j], dy = y[i] - y[j];
                    check_square(dx, &gen);
                    check_square(dy, &gen);
                    if ((i + j + b) % 3 == 0) sums.push_back(pow_fn(dx, 2) + pow_fn(dy, 2));
                }
        }
    }

    // (2) everything else (not part of the flagged share)
    Tally other;
    check_square(0.0, &other);
    check_square(-0.0, &other);
    for (int i = -2000; i <= 2000; ++i) {  // integer-valued and lattice coordinates
        check_square((double)i, &other);
        check_square(i * 0.25, &other);
        check_square(i * 0.1 - 0.3, &other);
        check_square((double)i * 1048576.0 + 1.0, &other);
    }
    for (int e = -1000; e <= 1000; ++e) {  // around powers of two, of the value and of its square
        const double b2 = std::ldexp(1.0, e), rt = std::ldexp(std::sqrt(2.0), e);
        double lo = b2, hi = b2, rlo = rt, rhi = rt;
        for (int k = 0; k < 40; ++k) {
            check_square(lo, &other);
            check_square(hi, &other);
            check_square(rlo, &other);
            check_square(rhi, &other);
            lo = std::nextafter(lo, 0.0);
            hi = std::nextafter(hi, INFINITY);
            rlo = std::nextafter(rlo, 0.0);
            rhi = std::nextafter(rhi, INFINITY);
        }
    }
    for (int k = 0; k < 200000; ++k) {  // tiny (< 2^-460) and huge (> 2^510) differences
        const double m = 1.0 + frand();
        check_square(std::ldexp(m, -461 - k % 600), &other);
        check_square(-std::ldexp(m, 510 + k % 514), &other);
    }
    check_square(DBL_MAX, &other);
    check_square(DBL_MIN, &other);
    check_square(std::ldexp(1.0, -1074), &other);
    check_square(INFINITY, &other);
    check_square(NAN, &other);
    if (other.differ == 0 && gen.differ == 0) fail("no pow(dx,2) != dx*dx anywhere", 0, 0, 0);

    // (3) sqrt_rn: sums of two squares, perfect squares, powers of four and
    // their neighbours, tiny and huge sums, the special values
    for (double a : sums) check_sqrt(a);
    for (int k = 0; k < 300000; ++k) {
        const double i = (double)(1 + std::rand() % 94906265);  // i*i < 2^53: exact
        check_sqrt(i * i);
        check_sqrt(std::ldexp(i * i, 2 * (k % 400 - 200)));
        check_sqrt(std::nextafter(i * i, 0.0));
        check_sqrt(std::nextafter(i * i, INFINITY));
        const double t = std::ldexp(1.0 + frand(), -461 - k % 560), h = std::ldexp(1.0 + frand(), 505 + k % 6);
        check_sqrt(pow_fn(t, 2) + pow_fn(0.75 * t, 2));
        check_sqrt(pow_fn(h, 2) + pow_fn(0.5 * h, 2));
    }
    for (int e = -537; e <= 511; ++e) {
        const double p4 = std::ldexp(1.0, 2 * e);
        double lo = p4, hi = p4, lo2 = 2 * p4, hi2 = 2 * p4;
        for (int k = 0; k < 8; ++k) {
            check_sqrt(lo);
            check_sqrt(hi);
            check_sqrt(lo2);
            check_sqrt(hi2);
            lo = std::nextafter(lo, 0.0);
            hi = std::nextafter(hi, INFINITY);
            lo2 = std::nextafter(lo2, 0.0);
            hi2 = std::nextafter(hi2, INFINITY);
        }
    }
    check_sqrt(DBL_MAX);
    check_sqrt(DBL_MIN);
    check_sqrt(std::ldexp(1.0, -1074));
    check_sqrt(INFINITY);
    check_sqrt(NAN);
    const double z = tspgpu::sqrt_rn(0.0);
    if (dist_bits(z) != 0) fail("sqrt_rn(0) is not +0.0", 0.0, z, 0.0);

    const double share = 100.0 * (double)gen.flagged / (double)gen.values;
    if (gen.values < 10000000) fail("generator sample below 1e7", (double)gen.values, 0, 0);
    if (gen.differ < 1000) fail("fewer than 1000 values with pow(dx,2) != dx*dx", (double)gen.differ, 0, 0);
    if (!(share < 12.0)) fail("flagged share not below 12%", share, 0, 0);
    if (g_fail) {
        std::fprintf(stderr, "check_dist_exact: %lld failures\n", g_fail);
        return 1;
    }
    std::printf("check_dist_exact: ok (%lld generator differences: %lld with pow != x*x, %.2f%% flagged; %lld other "
                "differences; %lld square roots)\n",
                gen.values, gen.differ, share, other.values, g_sqrt);
    return 0;
}
