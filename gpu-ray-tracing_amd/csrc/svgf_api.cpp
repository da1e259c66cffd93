// svgf_api.cpp — the C-ABI of the variance-guided filter: mrt_svgf_accumulate and mrt_svgf_filter
// (include/mrt_svgf.h). Per export: the plan (temporal_plan.cpp for the accumulation, whose scalars
// it shares; svgf_plan.cpp for the filter), the pointer checks, the launches (svgf_kernel.hip).
// Everything is enqueued on the caller's stream; nothing waits on the host, nothing is allocated and
// no state outlives a call.
#include <cstdint>

#include "../../include/mrt_svgf.h"
#include "api_checks.hpp"
#include "api_common.hpp"
#include "svgf_kernel.hpp"
#include "svgf_plan.hpp"
#include "temporal_plan.hpp"

using mrt::aligned16;
using mrt::any_overlap;
using mrt::fail;
using mrt::launched;
using mrt::Span;

extern "C" {

int mrt_svgf_accumulate(const mrt_svgf_accumulate_params* q, void* stream) {
    if (!q) return fail(MRT_ERR_INVALID_ARG, "null params");
    const mrt::TemporalPlan plan =
        mrt::plan_temporal_accumulate(q->width, q->height, q->maxHistory, q->normalCos, q->sigmaPlane, q->variant);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    const bool havePrev = q->havePrev != 0;
    const void* const prevGuide = havePrev ? q->prevGuide : nullptr;   // ignored where there is no previous frame
    const float* const prevHistory = havePrev ? q->prevHistory : nullptr;
    const float* const prevMoments = havePrev ? q->prevMoments : nullptr;
    if (!q->image || !q->guide || !q->albedo || !q->history || !q->moments ||
        (havePrev && (!prevGuide || !prevHistory || !prevMoments)))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(q->image) || !aligned16(q->guide) || !aligned16(q->albedo) || !aligned16(q->prevPosition) ||
        !aligned16(prevGuide) || !aligned16(prevHistory) || !aligned16(prevMoments) || !aligned16(q->history) ||
        !aligned16(q->moments) || !aligned16(q->imageOut))
        return fail(MRT_ERR_INVALID_ARG, "a buffer other than pixels is not 16-byte aligned");
    const int64_t px = (int64_t)q->width * q->height;
    const Span ins[] = {{q->image, 16 * px},   {q->guide, 32 * px},    {q->albedo, 16 * px}, {q->prevPosition, 16 * px},
                        {prevGuide, 32 * px}, {prevHistory, 16 * px}, {prevMoments, 16 * px}};
    const Span outs[] = {{q->history, 16 * px}, {q->moments, 16 * px}, {q->imageOut, 16 * px}, {q->pixels, 4 * px}};
    if (any_overlap(ins, outs))
        return fail(MRT_ERR_INVALID_ARG, "history, moments, imageOut or pixels overlaps an input or another output");
    mrt::SvgfAccumulateLaunch a{};
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
    a.prevMoments = reinterpret_cast<const float4*>(prevMoments);
    a.history = reinterpret_cast<float4*>(q->history);
    a.moments = reinterpret_cast<float4*>(q->moments);
    a.imageOut = reinterpret_cast<float4*>(q->imageOut);
    a.pixels = q->pixels;
    const hipError_t e = mrt::launch_svgf_accumulate(a, plan.grid, plan.tiled != 0, static_cast<hipStream_t>(stream));
    return launched(e, "svgf accumulate launch");
}

int mrt_svgf_filter(const mrt_svgf_filter_params* q, void* stream) {
    if (!q) return fail(MRT_ERR_INVALID_ARG, "null params");
    const mrt::SvgfPlan plan = mrt::plan_svgf_filter(q->width, q->height, q->iterations, q->normalSquarings, q->sigmaLuminance,
                                                     q->sigmaPlane, q->variant);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    const int N = plan.iterations;
    float* const scratch0 = N >= 1 ? q->scratch[0] : nullptr;   // an iteration count that does not use one
    float* const scratch1 = N >= 2 ? q->scratch[1] : nullptr;   // ignores it
    if (!q->image || !q->guide || !q->albedo || !q->moments || (N >= 1 && !scratch0) || (N >= 2 && !scratch1))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!q->imageOut && !q->pixels) return fail(MRT_ERR_INVALID_ARG, "neither imageOut nor pixels");
    if (!aligned16(q->image) || !aligned16(q->guide) || !aligned16(q->albedo) || !aligned16(q->moments) ||
        !aligned16(scratch0) || !aligned16(scratch1) || !aligned16(q->imageOut))
        return fail(MRT_ERR_INVALID_ARG, "image, guide, albedo, moments, scratch or imageOut not 16-byte aligned");
    const int64_t px = (int64_t)q->width * q->height;
    const Span ins[] = {{q->image, 16 * px}, {q->guide, 32 * px}, {q->albedo, 16 * px}, {q->moments, 16 * px}};
    const Span outs[] = {{scratch0, 16 * px}, {scratch1, 16 * px}, {q->imageOut, 16 * px}, {q->pixels, 4 * px},
                         {q->varianceOut, 4 * px}};
    if (any_overlap(ins, outs)) return fail(MRT_ERR_INVALID_ARG, "an output or scratch buffer overlaps an input or another output");
    mrt::SvgfFilterLaunch a{};
    a.width = q->width;
    a.height = q->height;
    a.squarings = q->normalSquarings;
    a.invPlane = plan.invPlane;
    a.sigmaLum2 = plan.sigmaLum2;
    a.image = reinterpret_cast<const float4*>(q->image);
    a.guide = static_cast<const float4*>(q->guide);
    a.albedo = reinterpret_cast<const float4*>(q->albedo);
    a.moments = reinterpret_cast<const float4*>(q->moments);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* const pingpong[2] = {scratch0, scratch1};
    // launch 0 is the variance launch, launch k + 1 iteration k; launch j < N writes pingpong[j & 1]
    hipError_t e = hipSuccess;
    for (int j = 0; j <= N && e == hipSuccess; j++) {
        a.last = j == N;
        a.in = j == 0 ? nullptr : reinterpret_cast<const float4*>(pingpong[(j - 1) & 1]);
        a.out = reinterpret_cast<float4*>(a.last ? q->imageOut : pingpong[j & 1]);
        a.pixels = a.last ? q->pixels : nullptr;
        a.varianceOut = a.last ? q->varianceOut : nullptr;
        if (j == 0) {
            a.tilesX = plan.varianceTilesX;
            e = mrt::launch_svgf_variance(a, plan.varianceGrid, s);
            continue;
        }
        const mrt::SvgfLaunchPlan& it = plan.at[j - 1];
        a.step = it.step;
        a.tilesX = it.tilesX;
        a.residues = it.residues;
        if (it.tiled) e = mrt::launch_svgf_iterate_tiled(a, it.grid, it.ldsBytes, s);
        else e = mrt::launch_svgf_iterate(a, it.grid, s);
    }
    return launched(e, "svgf filter launch");
}

}  // extern "C"
