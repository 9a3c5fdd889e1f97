// K1-wide on int32 distances (the integer-weight extension): the int32_t
// instantiation of hkwide_impl.h behind tspgpu_solve_instance_i32 — integer
// add and min, INT_MAX sentinel, a table of half the bytes.  Every candidate
// is an exact sum of at most n weights with n * max(d) < INT_MAX, so nothing
// overflows and the DP takes the decisions of the f64 DP on the same matrix.
#include "hkwide_impl.h"

using namespace tspgpu_wide;

extern "C" {

int tspgpu_solve_instance_i32(tspgpu_ctx *c, const int32_t *dist, int n, int32_t *cost_out, int32_t *tour_out,
                              double *kernel_ms)
{
    if (!c || !dist || !cost_out || !tour_out) return -EINVAL;
    if (n < 3 || n > kWideMaxN + 1) return -EINVAL;
    // (tspgpu_validate_i32 caps n at 20: the same checks on the values here)
    int64_t mx = 0;
    for (int i = 0; i < n * n; ++i) {
        if (dist[i] < 0) return -EINVAL;
        if (dist[i] > mx) mx = dist[i];
    }
    if ((int64_t)n * mx >= (int64_t)INT_MAX) return -ERANGE;
    return solve_wide<int32_t>(c, dist, n, cost_out, tour_out, kernel_ms);
}

}  // extern "C"
