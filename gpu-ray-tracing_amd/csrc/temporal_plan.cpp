// temporal_plan.cpp — the temporal accumulation's plan (temporal_plan.hpp). The order of the checks is
// the order include/mrt_temporal.h documents: shape (MRT_ERR_INVALID_ARG), limits
// (MRT_ERR_TOO_LARGE), then empty.
#include "temporal_plan.hpp"

#include "../../include/mrt.h"

namespace mrt {
namespace {

TemporalPlan refuse(int rc, const char* why) {
    TemporalPlan p{};
    p.rc = rc;
    p.why = why;
    return p;
}

}  // namespace

TemporalPlan plan_temporal_motion(int32_t numPrimary, int64_t numTris, int64_t numVertices, int32_t numPixels) {
    if (numPrimary < 0 || numTris < 0 || numVertices < 0 || numPixels < 0)
        return refuse(MRT_ERR_INVALID_ARG, "temporal motion: negative count");
    if (numPrimary > temporal::kMaxPixels || numPixels > temporal::kMaxPixels)
        return refuse(MRT_ERR_TOO_LARGE, "temporal motion: more than 2^26 slots or pixels");
    TemporalPlan p{};
    p.rc = MRT_OK;
    p.why = "";
    p.empty = numPrimary == 0 || numPixels == 0;
    p.grid = (int)(((int64_t)numPrimary + temporal::kThreads - 1) / temporal::kThreads);
    return p;
}

TemporalPlan plan_temporal_accumulate(int32_t width, int32_t height, int32_t maxHistory, float normalCos, float sigmaPlane,
                                      int32_t variant) {
    if (width < 1 || height < 1 || maxHistory < 1 || variant < 0 || variant > 2)
        return refuse(MRT_ERR_INVALID_ARG, "temporal accumulate: bad frame size, history length or variant");
    if (!(sigmaPlane > 0.0f) || normalCos != normalCos)   // a NaN sigmaPlane compares false
        return refuse(MRT_ERR_INVALID_ARG, "temporal accumulate: sigmaPlane must be above 0 and normalCos a number");
    if ((int64_t)width * height > temporal::kMaxPixels)
        return refuse(MRT_ERR_TOO_LARGE, "temporal accumulate: more than 2^26 pixels");
    if (maxHistory > temporal::kMaxHistory) return refuse(MRT_ERR_TOO_LARGE, "temporal accumulate: maxHistory above 2^20");
    TemporalPlan p{};
    p.rc = MRT_OK;
    p.why = "";
    p.invPlane = 1.0f / sigmaPlane;
    p.tiled = variant == 0 ? temporal::kDefaultTiled : (variant == 2 ? 1 : 0);
    if (p.tiled) {
        p.tilesX = (width + temporal::kTileW - 1) / temporal::kTileW;
        p.tilesY = (height + temporal::kTileH - 1) / temporal::kTileH;
        p.grid = p.tilesX * p.tilesY;   // < 2^26 / 256 + 2^26 / 32 + 2^26 / 8 + 1
    } else {
        p.grid = (int)(((int64_t)width * height + temporal::kThreads - 1) / temporal::kThreads);
    }
    return p;
}

}  // namespace mrt
