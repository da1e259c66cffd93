// denoise_plan.hpp — what the denoiser's C-ABI (denoise_api.cpp) and its host statement
// (host/denoise.cpp) decide before they touch anything: the scalar checks and limits of a call, the
// per-iteration constants, the grids and the tile geometry. Plain C++ with no HIP in it (the host
// compiler builds denoise_plan.cpp), so tests/cpp/denoise_driver.cpp runs it on the CPU.
#pragma once
#include <cstdint>

#include "denoise_limits.hpp"

namespace mrt {

// One launch of the filter. Direct: tilesX x tilesY tiles of denoise::kTileW x kTileH pixels. Staged
// (tiled != 0): tilesX tiles of denoise::kRowTileW columns; tilesY = residues * groups, the tile of
// residue r and group g holding the rows r + step * (kRowTileRows * g + j), j < kRowTileRows.
struct DenoiseLaunchPlan {
    int step;          // 1 << k
    int tiled;         // the LDS-staged kernel, else the direct one
    int grid;          // tilesX * tilesY workgroups of denoise::kThreads lanes
    int tilesX, tilesY;
    int residues;      // staged only: min(step, height)
    int ldsBytes;      // staged only: kRowTileStaged * (kRowTileW + 4 * step) * kRecordBytes
    float invColor2;   // 1 / (s * s), s = sigmaColor * 2^-k, all in float32
};

struct DenoisePlan {
    int rc;            // MRT_OK, or the error the call returns before it touches anything
    const char* why;
    bool empty;        // features only: no slot or no pixel: MRT_OK, nothing launched
    int grid;          // features only: workgroups of denoise::kThreads lanes
    int launches;      // filter only: max(iterations, 1); iterations == 0: one direct-geometry launch
    float invPlane;    // 1 / sigmaPlane
    DenoiseLaunchPlan at[denoise::kMaxIterations];
};

DenoisePlan plan_denoise_features(int32_t numPrimary, int64_t numTris, int32_t numPixels);
// variant: 0 = the staged kernel at the steps where it was measured faster (<= kTiledDefaultMaxStep),
// 1 = the direct kernel at every step, 2 = the staged kernel wherever its tile fits (<= kTiledMaxStep).
DenoisePlan plan_denoise_filter(int32_t width, int32_t height, int32_t iterations, int32_t normalSquarings,
                                float sigmaColor, float sigmaPlane, int32_t variant);

}  // namespace mrt
