// svgf_plan.cpp — the variance-guided filter's plan (svgf_plan.hpp). The order of the checks is the
// order include/mrt_svgf.h documents: shape (MRT_ERR_INVALID_ARG), then limits (MRT_ERR_TOO_LARGE).
#include "svgf_plan.hpp"

#include "../../include/mrt.h"

namespace mrt {
namespace {

SvgfPlan refuse(int rc, const char* why) {
    SvgfPlan p{};
    p.rc = rc;
    p.why = why;
    return p;
}

}  // namespace

SvgfPlan plan_svgf_filter(int32_t width, int32_t height, int32_t iterations, int32_t normalSquarings, float sigmaLuminance,
                          float sigmaPlane, int32_t variant) {
    if (width < 1 || height < 1 || iterations < 0 || normalSquarings < 0 || variant < 0 || variant > 2)
        return refuse(MRT_ERR_INVALID_ARG, "svgf filter: bad frame size, iteration or squaring count, or variant");
    if (!(sigmaLuminance > 0.0f) || !(sigmaPlane > 0.0f))   // a NaN compares false
        return refuse(MRT_ERR_INVALID_ARG, "svgf filter: sigmaLuminance and sigmaPlane must be above 0");
    if ((int64_t)width * height > svgf::kMaxPixels) return refuse(MRT_ERR_TOO_LARGE, "svgf filter: more than 2^26 pixels");
    if (iterations > svgf::kMaxIterations) return refuse(MRT_ERR_TOO_LARGE, "svgf filter: more than 8 iterations");
    if (normalSquarings > svgf::kMaxSquarings) return refuse(MRT_ERR_TOO_LARGE, "svgf filter: more than 10 squarings");
    SvgfPlan p{};
    p.rc = MRT_OK;
    p.why = "";
    p.iterations = iterations;
    p.invPlane = 1.0f / sigmaPlane;
    p.sigmaLum2 = sigmaLuminance * sigmaLuminance;
    const int directX = (width + svgf::kTileW - 1) / svgf::kTileW, directY = (height + svgf::kTileH - 1) / svgf::kTileH;
    p.varianceTilesX = directX;
    p.varianceGrid = directX * directY;
    const int tiledMaxStep = variant == 1 ? 0 : (variant == 2 ? svgf::kTiledMaxStep : svgf::kTiledDefaultMaxStep);
    for (int k = 0; k < svgf::kMaxIterations; k++) {
        SvgfLaunchPlan& it = p.at[k];
        it.step = 1 << k;
        it.tiled = k < iterations && it.step <= tiledMaxStep;
        if (it.tiled) {
            const int rows = (height + it.step - 1) / it.step;   // of residue 0, which has the most
            it.residues = it.step < height ? it.step : height;
            it.tilesX = (width + svgf::kRowTileW - 1) / svgf::kRowTileW;
            it.tilesY = it.residues * ((rows + svgf::kRowTileRows - 1) / svgf::kRowTileRows);
            it.ldsBytes = svgf::kRowTileStaged * (svgf::kRowTileW + 4 * it.step) * svgf::kRecordBytes;
        } else {
            it.tilesX = directX;
            it.tilesY = directY;
        }
        it.grid = it.tilesX * it.tilesY;   // < 2^26 / 256 + 2^26 / 32 + 2^26 / 4 + 16
    }
    return p;
}

}  // namespace mrt
