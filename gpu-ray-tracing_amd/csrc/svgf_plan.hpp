// svgf_plan.hpp — what the variance-guided filter's C-ABI (svgf_api.cpp) and its host statement
// (host/svgf.cpp) decide before they touch anything: the scalar checks and limits of a call, the
// constants, the grids and the tile geometry. Plain C++ with no HIP in it (the host compiler builds
// svgf_plan.cpp), so tests/cpp/svgf_driver.cpp runs it on the CPU. mrt_svgf_accumulate has the
// scalars of mrt_temporal_accumulate and takes its plan: plan_temporal_accumulate (temporal_plan.hpp).
#pragma once
#include <cstdint>

#include "svgf_limits.hpp"

namespace mrt {

// One iteration's launch. Direct: tilesX x tilesY tiles of svgf::kTileW x kTileH pixels. Staged
// (tiled != 0): DenoiseLaunchPlan's geometry: tilesX tiles of svgf::kRowTileW columns; tilesY =
// residues * groups, the tile of residue r and group g holding the rows r + step * (kRowTileRows *
// g + j), j < kRowTileRows.
struct SvgfLaunchPlan {
    int step;          // 1 << k
    int tiled;         // the LDS-staged kernel, else the direct one
    int grid;          // tilesX * tilesY workgroups of svgf::kThreads lanes
    int tilesX, tilesY;
    int residues;      // staged only: min(step, height)
    int ldsBytes;      // staged only: kRowTileStaged * (kRowTileW + 4 * step) * kRecordBytes
};

struct SvgfPlan {
    int rc;            // MRT_OK, or the error the call returns before it touches anything
    const char* why;
    int iterations;    // launches: 1 + iterations
    int varianceGrid, varianceTilesX;   // the variance launch: direct geometry
    float invPlane;    // 1 / sigmaPlane
    float sigmaLum2;   // sigmaLuminance * sigmaLuminance
    SvgfLaunchPlan at[svgf::kMaxIterations];
};

// Checks, in this order: width or height < 1, a negative iterations or normalSquarings, a variant
// outside 0..2, a sigmaLuminance or sigmaPlane that is not above 0 (MRT_ERR_INVALID_ARG); more than
// 2^26 pixels, 8 iterations or 10 squarings (MRT_ERR_TOO_LARGE). variant: 0 = the staged kernel at
// steps <= kTiledDefaultMaxStep, 1 = the direct kernel at every step, 2 = the staged kernel wherever
// its tile fits (<= kTiledMaxStep).
SvgfPlan plan_svgf_filter(int32_t width, int32_t height, int32_t iterations, int32_t normalSquarings, float sigmaLuminance,
                          float sigmaPlane, int32_t variant);

}  // namespace mrt
