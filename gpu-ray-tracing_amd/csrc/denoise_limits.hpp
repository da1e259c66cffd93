// denoise_limits.hpp — the sizes the denoiser's kernels (denoise_kernel.hip) are written for and its
// plan (denoise_plan.cpp) sizes grids by: one copy. Plain C++ with no HIP in it.
#pragma once
#include <cstdint>

namespace mrt {
namespace denoise {

constexpr int kThreads = 256;             // workgroup of both kernels
constexpr int kTileW = 32, kTileH = 8;    // the filter's workgroup: a 32 x 8 block of pixels, one lane each
// The LDS-staged filter's workgroup: 64 consecutive columns of 4 rows `step` apart, one lane each, with
// a halo of 2 * step columns on each side and 2 rows (of the same residue) above and below.
constexpr int kRowTileW = 64, kRowTileRows = 4, kRowTileStaged = kRowTileRows + 4;
constexpr int kRecordBytes = 48;          // a staged pixel: its guide (32) and its colour (16)
constexpr int kTiledMaxStep = 16;         // the widest step staged: 8 x (64 + 4 * 16) x 48 = 48 KB of LDS
constexpr int kTiledDefaultMaxStep = 16;  // the widest step at which the staged kernel ships
constexpr int64_t kMaxPixels = 1 << 26;   // width * height of a frame, and the slots of a features call
constexpr int kMaxIterations = 8;         // steps 1 .. 128
constexpr int kMaxSquarings = 10;         // the normal weight's exponent 2^10

static_assert(kTileW * kTileH == kThreads && kRowTileW * kRowTileRows == kThreads, "one lane per pixel of the tile");
static_assert(kRowTileStaged * (kRowTileW + 4 * kTiledMaxStep) * kRecordBytes <= 64 * 1024, "the tile fits the default LDS limit");

}  // namespace denoise
}  // namespace mrt
