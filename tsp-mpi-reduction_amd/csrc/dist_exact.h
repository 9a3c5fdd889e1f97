// The exactness rules of the device distance build, one copy
// for the kernels (cities.hip) and for the host (host/check_dist_exact.cpp).
//
// The reference's computeDistanceMatrix (assignment2.h:184-200) is
// sqrt(pow(dx, 2) + pow(dy, 2)) with glibc's pow and sqrt.  sqrt is correctly
// rounded; pow is not, and pow(x, 2) differs from x*x for ~0.08% of inputs.
// These two functions let a device compute the same bits: square_needs_host
// says for which dx the product dx*dx is certainly pow(dx, 2) (the others go
// to the host's pow), and sqrt_rn is a correctly rounded sqrt that does not
// depend on the device's.
//
// Every unit that includes this is built with -ffp-contract=off: the products
// and sums below must round where they are written.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TSPGPU_DIST_HD __host__ __device__ inline
#else
#define TSPGPU_DIST_HD inline
#endif

namespace tspgpu {

TSPGPU_DIST_HD uint64_t dist_bits(double v)
{
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}

TSPGPU_DIST_HD double dist_from_bits(uint64_t u)
{
    double v;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

// ulp of a finite v with |v| >= 2^-970 (the callers' ranges): 2^(exponent - 52)
TSPGPU_DIST_HD double dist_ulp(double v)
{
    const uint64_t e = (dist_bits(v) >> 52) & 0x7ffu;
    return dist_from_bits((e - 52) << 52);
}

TSPGPU_DIST_HD bool dist_is_pow2(double v) { return (dist_bits(v) & 0x000fffffffffffffull) == 0; }

// *p = dx*dx.  false: pow(dx, 2) == *p for certain; true: ask the host's pow.
//
// With p = fl(dx*dx) the exact square is p + r, r = fma(dx, dx, -p) (exact:
// the error of a product is a double while nothing underflows).  pow can only
// return another double than p when the exact square lies close enough to the
// midpoint between p and its neighbour on r's side: that neighbour is
// 2g - |r| away, g being half the gap (ulp(p)/2, or ulp(p)/4 below a power of
// two, where the spacing halves).  glibc's pow (sysdeps/ieee754/dbl-64/e_pow.c,
// since 2.28) documents a worst-case error of 0.52-0.54 ULP in round-to-
// nearest, i.e. at most 0.54 * 2g from the exact value.  The rule flags
// |r| >= 0.9 g, so an unflagged square keeps the neighbour more than
// 1.1 g = 0.55 gaps away: the 0.9 margin covers a pow error of up to 0.55 ULP,
// one hundredth above the documented bound.  It flags 10% of the generator's
// coordinate differences (0.45 <= |r| / ulp <= 0.5), a superset of the 0.08%
// where pow really differs (host/check_dist_exact.cpp counts both).
//
// Squares outside [2^-900, 2^1000], infinities and NaNs go to the host too
// (r is not exact there, and pow's special cases are its own); dx == 0 gives
// +0.0 like pow(+-0, 2).
TSPGPU_DIST_HD bool square_needs_host(double dx, double *p)
{
    const double sq = dx * dx;
    *p = sq;
    if (dx == 0.0) return false;
    if (!(sq >= 0x1p-900 && sq <= 0x1p1000)) return true;
    const double r = fma(dx, dx, -sq);
    double g = 0.5 * dist_ulp(sq);
    if (r < 0.0 && dist_is_pow2(sq)) g *= 0.5;
    return fabs(r) >= 0.9 * g;
}

// sqrt(a) correctly rounded (the bits of glibc's sqrt), whatever the rounding
// of the sqrt it starts from: with s = sqrt(a), the candidate c among s and
// its two neighbours is the answer iff a lies between the squared midpoints
// around c, -c*u < a - c*c <= c*u with u = ulp(c) (the lower bound is -c*u/2
// for a power of two c: the spacing below it is u/2).  a - c*c is a multiple
// of u*u of at most 53 bits, so one fma gives it exactly, and the midpoints'
// u*u/4 terms fall between two such multiples.  a below
// 2^-900 is scaled by 2^200 first (the residual would underflow; the scaling
// is exact and sqrt scales by 2^100).  a == 0 gives +0.0; infinities and NaNs
// pass through (such a block fails validation later).
//
// sqrt_rn_accepts is that test for one candidate c > 0 (a finite, >= 2^-900).
TSPGPU_DIST_HD bool sqrt_rn_accepts(double c, double a)
{
    const double e = fma(-c, c, a);
    const double hi = c * dist_ulp(c);
    const double lo = dist_is_pow2(c) ? -0.5 * hi : -hi;
    return lo < e && e <= hi;
}

TSPGPU_DIST_HD double sqrt_rn(double a)
{
    if (a == 0.0) return 0.0;
    if (!(a > 0.0 && a <= 0x1.fffffffffffffp1023)) return a < 0.0 ? sqrt(a) : a;
    const bool tiny = a < 0x1p-900;
    if (tiny) a *= 0x1p200;
    const double s = sqrt(a);
    const double u = dist_ulp(s);
    double out = s;
    if (!sqrt_rn_accepts(s, a)) {
        const double below = s - (dist_is_pow2(s) ? 0.5 * u : u), above = s + u;
        if (sqrt_rn_accepts(below, a))
            out = below;
        else if (sqrt_rn_accepts(above, a))
            out = above;
    }
    return tiny ? out * 0x1p-100 : out;
}

}  // namespace tspgpu
