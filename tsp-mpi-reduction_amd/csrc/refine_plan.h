// Host plan of the window refinement (tspgpu_refine_path*, include/tspgpu.h,
// DESIGN.md §6d): which windows a pass solves and when the passes stop.  Pure
// host code, no HIP (built into libtspgpu.so and, with host/check_refine.cpp,
// into a stand-alone program under ASan + UBSan: make check-refine).
//
// A path of L cities is tiled by windows of w = m + 2 positions: m interior
// positions between two fixed ends, consecutive windows sharing an end, so
// window k of a pass starts at offset + k * (m + 1).  Even passes start at 0,
// odd passes half a window later, which moves every seam of one pass into a
// window interior of the next.
#pragma once
#include <cstdint>

namespace tspgpu {

constexpr int kRefineMinM = 2;
constexpr int kRefineMaxM = 18;        // w = 20 = TSPGPU_MAX_CITIES
constexpr int kRefineStrictMaxM = 15;  // w = 17: K1 on 16 cities

struct RefinePass {
    int64_t offset = 0;   // position of window 0's fixed start
    int64_t windows = 0;  // W: windows of the pass (0: an empty pass)
    int64_t stride = 0;   // m + 1: start of window k = offset + k * stride
    int w = 0;            // m + 2 positions per window
    int64_t cities = 0;   // W * w: the gathered copy
    int64_t dist = 0;     // W * w * w: the windows' matrices (elements)
    int64_t fold = 0;     // W * (w-1) * (w-1): the folded matrices K1 solves
};

// 0, or -EINVAL: L < 2, m outside [2, 18] (strict: 15), pass < 0, or more
// windows than an int holds (K1's block count)
int refine_pass(int64_t L, int m, int pass, int strict, RefinePass *out);

// The stop rule after pass `pass` (0-based): the last allowed pass, or two
// passes in a row (this one and the one before) that replaced no window.
bool refine_stop(int pass, int max_passes, int64_t replaced, int64_t replaced_before);

}  // namespace tspgpu
