// temporal.cpp — the temporal accumulation on the CPU: the statements mrt_temporal_motion /
// mrt_temporal_accumulate (csrc/temporal_kernel.hip) are checked against, term for term
// (csrc/temporal_common.hpp), with the device's plan (csrc/temporal_plan.cpp: the same checks,
// limits and 1 / sigmaPlane). The slots and the pixels are walked in order.
#include <cstring>

#include "../../../include/mrt_host.h"
#include "../temporal_common.hpp"
#include "../temporal_plan.hpp"
#include "host_error.hpp"
#include "records.hpp"

namespace mrt {
namespace {

static_assert(sizeof(rg::RayRec) == 32 && sizeof(temporal::Guide) == 32 && sizeof(temporal::Color) == 16, "record sizes");

struct TemporalHostSource {
    const mrth_temporal_params& a;
    temporal::Color image(int p) const { return get_record<temporal::Color>(a.image, p); }
    temporal::Guide guide(int p) const { return get_record<temporal::Guide>(a.guide, p); }
    temporal::Color albedo(int p) const { return get_record<temporal::Color>(a.albedo, p); }
    temporal::Color prev_position(int p) const { return get_record<temporal::Color>(a.prevPosition, p); }
    temporal::Guide prev_guide(int q) const { return get_record<temporal::Guide>(a.prevGuide, q); }
    temporal::Color prev_history(int q) const { return get_record<temporal::Color>(a.prevHistory, q); }
};

}  // namespace
}  // namespace mrt

extern "C" {

int mrth_temporal_motion(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                         const void* primaryResults, const int32_t* triangles, int64_t numTris, const float* vertices,
                         const float* prevVertices, int64_t numVertices, int32_t numPixels, float* prevPosition) {
    const mrt::TemporalPlan plan = mrt::plan_temporal_motion(numPrimary, numTris, numVertices, numPixels);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    if (plan.empty) return MRTH_OK;
    if (!primarySlotToId || !primaryRays || !primaryResults || !prevPosition || (numTris > 0 && !triangles) ||
        (numTris > 0 && numVertices > 0 && (!vertices || !prevVertices)))
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "temporal_motion: null argument");
    for (int32_t i = 0; i < numPrimary; i++) {
        const int32_t p = primarySlotToId[i];
        if (p < 0 || p >= numPixels) continue;
        const mrt::RayResult res = mrt::get_record<mrt::RayResult>(primaryResults, i);
        mrt::put_record(prevPosition, p,
                        mrt::temporal::motion_one(mrt::get_record<mrt::rg::RayRec>(primaryRays, i), res.id, res.t, triangles,
                                                  numTris, vertices, prevVertices, numVertices));
    }
    return MRTH_OK;
}

int mrth_temporal_accumulate(const mrth_temporal_params* a) {
    if (!a) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "temporal_accumulate: null params");
    const mrt::TemporalPlan plan =
        mrt::plan_temporal_accumulate(a->width, a->height, a->maxHistory, a->normalCos, a->sigmaPlane, a->variant);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    const bool havePrev = a->havePrev != 0;
    if (!a->image || !a->guide || !a->albedo || !a->history || (havePrev && (!a->prevGuide || !a->prevHistory)))
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "temporal_accumulate: null argument");
    mrt::temporal::Constants k{};
    k.width = a->width;
    k.height = a->height;
    k.havePrev = havePrev ? 1 : 0;
    k.maxHistory = a->maxHistory;
    k.hasPrevPosition = a->prevPosition ? 1 : 0;
    k.normalCos = a->normalCos;
    k.invPlane = plan.invPlane;
    for (int i = 0; i < 16; i++) k.m[i] = a->prevWorldToScreen[i];
    k.subpixel[0] = a->prevSubpixel[0];
    k.subpixel[1] = a->prevSubpixel[1];
    const mrt::TemporalHostSource src{*a};
    const int n = a->width * a->height;
    for (int p = 0; p < n; p++) {
        mrt::temporal::Color history, result;
        mrt::temporal::accumulate_pixel(src, k, p, history, result);
        mrt::put_record(a->history, p, history);
        if (a->imageOut) mrt::put_record(a->imageOut, p, result);
        if (a->pixels) a->pixels[p] = mrt::denoise::pixel_of(result);
    }
    return MRTH_OK;
}

}  // extern "C"
