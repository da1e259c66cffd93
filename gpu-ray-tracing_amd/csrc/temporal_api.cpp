// temporal_api.cpp — the C-ABI of the temporal accumulation: mrt_temporal_motion and
// mrt_temporal_accumulate (include/mrt_temporal.h). Per export: the plan (temporal_plan.cpp: scalar
// checks, limits, 1 / sigmaPlane, the grid), the pointer checks, the launch (temporal_kernel.hip).
// Everything is enqueued on the caller's stream; nothing waits on the host, nothing is allocated and
// no state outlives a call.
#include <cstdint>

#include "../../include/mrt_temporal.h"
#include "api_checks.hpp"
#include "api_common.hpp"
#include "temporal_kernel.hpp"
#include "temporal_plan.hpp"

using mrt::aligned16;
using mrt::any_overlap;
using mrt::fail;
using mrt::launched;
using mrt::Span;

extern "C" {

int mrt_temporal_motion(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                        const void* primaryResults, const int32_t* triangles, int64_t numTris, const float* vertices,
                        const float* prevVertices, int64_t numVertices, int32_t numPixels, float* prevPosition, void* stream) {
    const mrt::TemporalPlan plan = mrt::plan_temporal_motion(numPrimary, numTris, numVertices, numPixels);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    if (plan.empty) return MRT_OK;
    if (!primarySlotToId || !primaryRays || !primaryResults || !prevPosition || (numTris > 0 && !triangles) ||
        (numTris > 0 && numVertices > 0 && (!vertices || !prevVertices)))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(primaryRays) || !aligned16(primaryResults) || !aligned16(prevPosition))
        return fail(MRT_ERR_INVALID_ARG, "rays, results or prevPosition not 16-byte aligned");
    const int64_t n = numPrimary;
    const Span ins[] = {{primarySlotToId, 4 * n}, {primaryRays, 32 * n},        {primaryResults, 16 * n},
                        {triangles, 12 * numTris}, {vertices, 12 * numVertices}, {prevVertices, 12 * numVertices}};
    const Span outs[] = {{prevPosition, 16 * (int64_t)numPixels}};
    if (any_overlap(ins, outs)) return fail(MRT_ERR_INVALID_ARG, "prevPosition overlaps an input");
    mrt::TemporalMotionLaunch a{};
    a.numPrimary = numPrimary;
    a.numPixels = numPixels;
    a.numTris = numTris;
    a.numVertices = numVertices;
    a.primarySlotToId = primarySlotToId;
    a.primaryRays = static_cast<const mrt::rg::RayRec*>(primaryRays);
    a.primaryResults = static_cast<const int4*>(primaryResults);
    a.triangles = triangles;
    a.vertices = vertices;
    a.prevVertices = prevVertices;
    a.prevPosition = reinterpret_cast<float4*>(prevPosition);
    const hipError_t e = mrt::launch_temporal_motion(a, plan.grid, static_cast<hipStream_t>(stream));
    return launched(e, "temporal motion launch");
}

int mrt_temporal_accumulate(const mrt_temporal_params* q, void* stream) {
    if (!q) return fail(MRT_ERR_INVALID_ARG, "null params");
    const mrt::TemporalPlan plan =
        mrt::plan_temporal_accumulate(q->width, q->height, q->maxHistory, q->normalCos, q->sigmaPlane, q->variant);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    const bool havePrev = q->havePrev != 0;
    const void* const prevGuide = havePrev ? q->prevGuide : nullptr;   // ignored where there is no previous frame
    const float* const prevHistory = havePrev ? q->prevHistory : nullptr;
    if (!q->image || !q->guide || !q->albedo || !q->history || (havePrev && (!prevGuide || !prevHistory)))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(q->image) || !aligned16(q->guide) || !aligned16(q->albedo) || !aligned16(q->prevPosition) ||
        !aligned16(prevGuide) || !aligned16(prevHistory) || !aligned16(q->history) || !aligned16(q->imageOut))
        return fail(MRT_ERR_INVALID_ARG, "image, guide, albedo, prevPosition, prevGuide, prevHistory, history or imageOut not 16-byte aligned");
    const int64_t px = (int64_t)q->width * q->height;
    const Span ins[] = {{q->image, 16 * px},   {q->guide, 32 * px},    {q->albedo, 16 * px},
                        {q->prevPosition, 16 * px}, {prevGuide, 32 * px}, {prevHistory, 16 * px}};
    const Span outs[] = {{q->history, 16 * px}, {q->imageOut, 16 * px}, {q->pixels, 4 * px}};
    if (any_overlap(ins, outs)) return fail(MRT_ERR_INVALID_ARG, "history, imageOut or pixels overlaps an input or another output");
    mrt::TemporalAccumulateLaunch a{};
    a.k.width = q->width;
    a.k.height = q->height;
    a.k.havePrev = havePrev ? 1 : 0;
    a.k.maxHistory = q->maxHistory;
    a.k.hasPrevPosition = q->prevPosition ? 1 : 0;
    a.k.normalCos = q->normalCos;
    a.k.invPlane = plan.invPlane;
    for (int i = 0; i < 16; i++) a.k.m[i] = q->prevWorldToScreen[i];
    a.k.subpixel[0] = q->prevSubpixel[0];
    a.k.subpixel[1] = q->prevSubpixel[1];
    a.tilesX = plan.tilesX;
    a.image = reinterpret_cast<const float4*>(q->image);
    a.guide = static_cast<const float4*>(q->guide);
    a.albedo = reinterpret_cast<const float4*>(q->albedo);
    a.prevPosition = reinterpret_cast<const float4*>(q->prevPosition);
    a.prevGuide = static_cast<const float4*>(prevGuide);
    a.prevHistory = reinterpret_cast<const float4*>(prevHistory);
    a.history = reinterpret_cast<float4*>(q->history);
    a.imageOut = reinterpret_cast<float4*>(q->imageOut);
    a.pixels = q->pixels;
    const hipError_t e = mrt::launch_temporal_accumulate(a, plan.grid, plan.tiled != 0, static_cast<hipStream_t>(stream));
    return launched(e, "temporal accumulate launch");
}

}  // extern "C"
