// K1 variant 6 configuration 61 (a row of k1_cfg.h)
#include "hk_sub.h"
namespace tspgpu {
template hipError_t launch_sub_n<int32_t, 15, 10, 256, 8>(const SubArgs &);
}  // namespace tspgpu
