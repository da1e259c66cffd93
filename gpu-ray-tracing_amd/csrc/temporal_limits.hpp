// temporal_limits.hpp — the sizes the temporal accumulation's kernels (temporal_kernel.hip) are
// written for and its plan (temporal_plan.cpp) sizes grids by: one copy. Plain C++ with no HIP in it.
#pragma once
#include <cstdint>

namespace mrt {
namespace temporal {

constexpr int kThreads = 256;             // workgroup of both kernels
constexpr int kTileW = 32, kTileH = 8;    // the tiled accumulate shape: a 32 x 8 block of pixels, one lane each
constexpr int64_t kMaxPixels = 1 << 26;   // width * height of a frame, and the slots and pixels of a motion call
constexpr int kMaxHistory = 1 << 20;      // the longest running mean; a float counts it exactly
constexpr int kDefaultTiled = 0;          // variant 0's shape: the linear one; the tiled one did not win at every size measured

static_assert(kTileW * kTileH == kThreads, "one lane per pixel of the tile");

}  // namespace temporal
}  // namespace mrt
