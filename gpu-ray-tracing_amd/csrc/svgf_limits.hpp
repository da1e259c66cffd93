// svgf_limits.hpp — the sizes the variance-guided filter's kernels (svgf_kernel.hip) are written for
// and its plan (svgf_plan.cpp) sizes grids by: one copy. Plain C++ with no HIP in it. The fused
// accumulate's sizes are temporal_limits.hpp's.
#pragma once
#include <cstdint>

namespace mrt {
namespace svgf {

constexpr int kThreads = 256;             // workgroup of every kernel
constexpr int kTileW = 32, kTileH = 8;    // the variance launch's and the direct iteration's workgroup: 32 x 8 pixels
// The LDS-staged iteration's workgroup, as denoise_limits.hpp's: 64 consecutive columns of 4 rows
// `step` apart, with a halo of 2 * step columns on each side and 2 rows (of the same residue) above
// and below. A staged pixel is its guide (32 bytes) and its colour with the variance in w (16).
constexpr int kRowTileW = 64, kRowTileRows = 4, kRowTileStaged = kRowTileRows + 4;
constexpr int kRecordBytes = 48;
constexpr int kTiledMaxStep = 16;         // the widest step staged: 8 x (64 + 4 * 16) x 48 = 48 KB of LDS
constexpr int kTiledDefaultMaxStep = 8;   // the widest step at which the staged kernel ships: it won or tied at 1 .. 8, not at 16
constexpr int64_t kMaxPixels = 1 << 26;
constexpr int kMaxIterations = 8;         // steps 1 .. 128
constexpr int kMaxSquarings = 10;

static_assert(kTileW * kTileH == kThreads && kRowTileW * kRowTileRows == kThreads, "one lane per pixel of the tile");
static_assert(kRowTileStaged * (kRowTileW + 4 * kTiledMaxStep) * kRecordBytes <= 64 * 1024, "the tile fits the default LDS limit");

}  // namespace svgf
}  // namespace mrt
