// K1 large-batch configurations of variant 6 (hk_sub.h):
//   X(id, value type, N, L, threads, workgroups/CU)
// The first row per (N, value type) is the default; TSPGPU_TILED_CFG picks
// another by id.  A new row needs a matching k1/hks_p<id>.hip.
// 16 cities f64: 65 (eleven low cities, 512-thread workgroups) is 3.7% faster
// than 60 per 65536 blocks (profiles/l11_v6); 60 stays
// selectable.
//
// tests/test_k1_variants_gpu.py lists the configurations by reading this
// file: it finds a table by its #define line and takes the rows up to the
// next blank line.  The test suite of the commit before variant 5 was retired
// (8f46298) must keep running against this library, and it looks up both
// names below, so variant 5's keeps an empty table until that suite no
// longer has to run.
#pragma once
#include "hk_sub.h"

#define TSPGPU_TILED_PRODUCT_CFGS(X) /* variant 5: retired, no rows */

#define TSPGPU_SUB_PRODUCT_CFGS(X) \
    X(65, double, 15, 11, 512, 3) \
    X(60, double, 15, 10, 256, 6) \
    X(61, int32_t, 15, 10, 256, 8) \
    X(62, double, 14, 10, 256, 6) \
    X(63, double, 13, 10, 256, 6) \
    X(64, double, 12, 10, 256, 6)

namespace tspgpu {
struct SubCfg {
    int id, vbytes, N, L, threads, wg;
    hipError_t (*launch)(const SubArgs &);
};
#define TSPGPU_SUB_EXTERN(ID, V, N, L, T, W) extern template hipError_t launch_sub_n<V, N, L, T, W>(const SubArgs &);
TSPGPU_SUB_PRODUCT_CFGS(TSPGPU_SUB_EXTERN)
#undef TSPGPU_SUB_EXTERN
// every compiled configuration (tspgpu.cpp picks by n, value type and TSPGPU_TILED_CFG)
inline const SubCfg *sub_cfgs(int *count)
{
#define TSPGPU_SUB_ROW(ID, V, N, L, T, W) {ID, (int)sizeof(V), N, L, T, W, &launch_sub_n<V, N, L, T, W>},
    static const SubCfg t[] = {TSPGPU_SUB_PRODUCT_CFGS(TSPGPU_SUB_ROW)};
#undef TSPGPU_SUB_ROW
    *count = (int)(sizeof(t) / sizeof(t[0]));
    return t;
}
}  // namespace tspgpu
