// K1 variant 6 configuration 65 (a row of k1_cfg.h)
#include "hk_sub.h"
namespace tspgpu {
template hipError_t launch_sub_n<double, 15, 11, 512, 3>(const SubArgs &);
}  // namespace tspgpu
