// K1 variant 6 configuration 63 (a row of k1_cfg.h)
#include "hk_sub.h"
namespace tspgpu {
template hipError_t launch_sub_n<double, 13, 10, 256, 6>(const SubArgs &);
}  // namespace tspgpu
