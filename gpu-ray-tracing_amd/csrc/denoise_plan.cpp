// denoise_plan.cpp — the denoiser's plan (denoise_plan.hpp). The order of the checks is the order
// include/mrt.h documents: shape (MRT_ERR_INVALID_ARG), limits (MRT_ERR_TOO_LARGE), then empty.
#include "denoise_plan.hpp"

#include "../../include/mrt.h"

namespace mrt {
namespace {

DenoisePlan refuse(int rc, const char* why) {
    DenoisePlan p{};
    p.rc = rc;
    p.why = why;
    return p;
}

}  // namespace

DenoisePlan plan_denoise_features(int32_t numPrimary, int64_t numTris, int32_t numPixels) {
    if (numPrimary < 0 || numTris < 0 || numPixels < 0)
        return refuse(MRT_ERR_INVALID_ARG, "denoise features: negative count");
    if (numPrimary > denoise::kMaxPixels || numPixels > denoise::kMaxPixels)
        return refuse(MRT_ERR_TOO_LARGE, "denoise features: more than 2^26 slots or pixels");
    DenoisePlan p{};
    p.rc = MRT_OK;
    p.why = "";
    p.empty = numPrimary == 0 || numPixels == 0;
    p.grid = (int)(((int64_t)numPrimary + denoise::kThreads - 1) / denoise::kThreads);
    return p;
}

DenoisePlan plan_denoise_filter(int32_t width, int32_t height, int32_t iterations, int32_t normalSquarings,
                                float sigmaColor, float sigmaPlane, int32_t variant) {
    if (width < 1 || height < 1 || iterations < 0 || normalSquarings < 0 || variant < 0 || variant > 2)
        return refuse(MRT_ERR_INVALID_ARG, "denoise filter: bad frame size, iteration or squaring count, or variant");
    if (!(sigmaColor > 0.0f) || !(sigmaPlane > 0.0f))   // a NaN compares false
        return refuse(MRT_ERR_INVALID_ARG, "denoise filter: sigmaColor and sigmaPlane must be above 0");
    if ((int64_t)width * height > denoise::kMaxPixels)
        return refuse(MRT_ERR_TOO_LARGE, "denoise filter: more than 2^26 pixels");
    if (iterations > denoise::kMaxIterations) return refuse(MRT_ERR_TOO_LARGE, "denoise filter: more than 8 iterations");
    if (normalSquarings > denoise::kMaxSquarings) return refuse(MRT_ERR_TOO_LARGE, "denoise filter: more than 10 squarings");
    DenoisePlan p{};
    p.rc = MRT_OK;
    p.why = "";
    p.launches = iterations > 0 ? iterations : 1;
    p.invPlane = 1.0f / sigmaPlane;
    const int tiledMaxStep = variant == 1 ? 0 : (variant == 2 ? denoise::kTiledMaxStep : denoise::kTiledDefaultMaxStep);
    float scale = 1.0f;   // 2^-k
    for (int k = 0; k < denoise::kMaxIterations; k++) {
        DenoiseLaunchPlan& it = p.at[k];
        it.step = 1 << k;
        it.tiled = iterations > 0 && it.step <= tiledMaxStep;
        if (it.tiled) {
            const int rows = (height + it.step - 1) / it.step;   // of residue 0, which has the most
            it.residues = it.step < height ? it.step : height;
            it.tilesX = (width + denoise::kRowTileW - 1) / denoise::kRowTileW;
            it.tilesY = it.residues * ((rows + denoise::kRowTileRows - 1) / denoise::kRowTileRows);
            it.ldsBytes = denoise::kRowTileStaged * (denoise::kRowTileW + 4 * it.step) * denoise::kRecordBytes;
        } else {
            it.tilesX = (width + denoise::kTileW - 1) / denoise::kTileW;
            it.tilesY = (height + denoise::kTileH - 1) / denoise::kTileH;
        }
        it.grid = it.tilesX * it.tilesY;   // < 2^26 / 256 + 2^26 / 32 + 2^26 / 4 + 16
        const float s = sigmaColor * scale;
        const float s2 = s * s;
        it.invColor2 = 1.0f / s2;   // s2 overflows: 0 (the colour term is off); underflows to 0: infinity
        scale = scale * 0.5f;
    }
    return p;
}

}  // namespace mrt
