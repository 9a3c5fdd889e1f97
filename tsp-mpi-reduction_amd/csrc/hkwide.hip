// K1-wide on the reference's f64 distances: the double instantiation of
// hkwide_impl.h (kernels, workspace, launch sequence) behind
// tspgpu_solve_instance.  The int32 instantiation lives in hkwide_i32.hip, a
// code object of its own.
#include "hkwide_impl.h"

using namespace tspgpu_wide;

extern "C" {

int tspgpu_solve_instance(tspgpu_ctx *c, const double *dist, int n, double *cost_out, int32_t *tour_out,
                          double *kernel_ms)
{
    if (!c || !dist || !cost_out || !tour_out) return -EINVAL;
    if (n < 3 || n > kWideMaxN + 1) return -EINVAL;
    int rc = tspgpu_validate(dist, n, 1, 0 /* n <= 20 checked below */);
    if (rc == -EINVAL && n > TSPGPU_MAX_CITIES) {
        // tspgpu_validate caps n at 20: check the values here
        double mx = 0.0;
        for (int i = 0; i < n * n; ++i) {
            if (!(dist[i] >= 0.0) || std::signbit(dist[i]) || !(dist[i] < INFINITY)) return -EINVAL;
            mx = dist[i] > mx ? dist[i] : mx;
        }
        rc = (double)n * mx >= (double)INT_MAX ? -ERANGE : 0;
    }
    if (rc) return rc;
    return solve_wide<double>(c, dist, n, cost_out, tour_out, kernel_ms);
}

int tspgpu_wide_last_dtype(const tspgpu_ctx *c) { return c ? c->wide_last_dtype : -1; }

}  // extern "C"
