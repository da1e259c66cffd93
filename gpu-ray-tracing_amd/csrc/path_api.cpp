// path_api.cpp — the C-ABI of a path frame's steps around its traces: mrt_path_extend,
// mrt_path_accumulate and mrt_path_resolve. Per export: the plan (path_plan.cpp: scalar checks,
// limits, grids, scratch), the pointer checks, the launches (path_kernel.hip). Everything is
// enqueued on the caller's stream; nothing waits on the host and no state outlives a call.
#include <cstdint>

#include "api_checks.hpp"
#include "api_common.hpp"
#include "path_kernel.hpp"
#include "path_plan.hpp"

using mrt::aligned16;   // rays, states, pending contributions and radiances move as 16-byte words
using mrt::fail;
using mrt::hipFail;
using mrt::launched;
using mrt::Span;

extern "C" {

int mrt_path_extend(const mrt_path_extend_params* q, void* stream) {
    if (!q) return fail(MRT_ERR_INVALID_ARG, "null params");
    const mrt::PathPlan plan = mrt::plan_path_extend(q->vertex, q->depth, q->numSamples, q->numSlots, q->numPaths);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    if (plan.empty) return MRT_OK;
    const bool first = q->vertex == 0, last = q->vertex == q->depth;
    if (!q->triNormals || !q->triMaterialColor || !q->inRays || !q->inResults || (!first && !q->inState) ||
        !q->outShadowRays || !q->outPending || (!last && !q->outRays) || !q->outState || !q->radiance || !q->liveCount)
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (q->numTris < 0) return fail(MRT_ERR_INVALID_ARG, "negative triangle count");
    if (!aligned16(q->inRays) || !aligned16(q->outShadowRays) || !aligned16(q->outPending) || !aligned16(q->outState) ||
        !aligned16(q->radiance) || (!first && !aligned16(q->inState)) || (!last && !aligned16(q->outRays)))
        return fail(MRT_ERR_INVALID_ARG, "rays, states, pending or radiance not 16-byte aligned");
    const int64_t n = q->numSlots, inputs = first ? (n + q->numSamples - 1) / q->numSamples : n;
    const Span ins[] = {{q->inRays, 32 * inputs}, {q->inResults, 16 * inputs}, {first ? nullptr : q->inState, 16 * n}};
    const Span outs[] = {{q->outShadowRays, 32 * n}, {q->outPending, 16 * n}, {last ? nullptr : q->outRays, 32 * n},
                         {q->outState, 16 * n}, {q->radiance, 16 * (int64_t)q->numPaths}, {q->liveCount, 4}};
    if (mrt::output_overlaps_input(ins, outs)) return fail(MRT_ERR_INVALID_ARG, "an output buffer overlaps an input buffer");
    if (mrt::outputs_overlap(outs)) return fail(MRT_ERR_INVALID_ARG, "two output buffers overlap");
    mrt::PathExtendLaunch a{};
    a.p.vertex = q->vertex;
    a.p.depth = q->depth;
    a.p.numSamples = q->numSamples;
    a.p.seed = q->seed;
    for (int k = 0; k < 3; k++) {
        a.p.lightPos[k] = q->lightPos[k];
        a.p.lightColor[k] = q->lightColor[k];
        a.p.sky[k] = q->sky[k];
    }
    a.p.lightRadius = q->lightRadius;
    a.p.maxDist = q->maxDist;
    a.p.triNormals = q->triNormals;
    a.p.triMaterialColor = q->triMaterialColor;
    a.p.numTris = q->numTris;
    a.numSlots = q->numSlots;
    a.numPaths = q->numPaths;
    a.compact = q->compact != 0;
    a.inRays = static_cast<const mrt::rg::RayRec*>(q->inRays);
    a.inResults = static_cast<const int2*>(q->inResults);
    a.inState = static_cast<const mrt::path::State*>(q->inState);
    a.outShadow = static_cast<mrt::rg::RayRec*>(q->outShadowRays);
    a.outPending = static_cast<float4*>(q->outPending);
    a.outRays = static_cast<mrt::rg::RayRec*>(q->outRays);
    a.outState = static_cast<mrt::path::State*>(q->outState);
    a.radiance = reinterpret_cast<float4*>(q->radiance);
    a.liveCount = q->liveCount;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mrt::StreamScratch counts;
    if (hipError_t e = counts.alloc(plan.scratchBytes, s)) return hipFail(e, "hipMallocAsync(path counts)");
    a.counts = counts.as<int32_t>();
    hipError_t e = mrt::launch_path_count(a, plan.grid, s);
    if (e == hipSuccess) e = mrt::launch_path_scan(a.counts, plan.grid, a.liveCount, s);
    if (e == hipSuccess) e = mrt::launch_path_extend(a, plan.grid, s);
    return launched(e, "path extend launch", counts, "hipFreeAsync(path counts)");
}

int mrt_path_accumulate(int32_t numSlots, int32_t numPaths, const void* state, const void* pending,
                        const void* shadowResults, float* radiance, void* stream) {
    const mrt::PathPlan plan = mrt::plan_path_accumulate(numSlots, numPaths);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    if (plan.empty) return MRT_OK;
    if (!state || !pending || !shadowResults || !radiance) return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(state) || !aligned16(pending) || !aligned16(shadowResults) || !aligned16(radiance))
        return fail(MRT_ERR_INVALID_ARG, "states, pending, results or radiance not 16-byte aligned");
    mrt::PathAccumulateLaunch a{};
    a.numSlots = numSlots;
    a.numPaths = numPaths;
    a.state = static_cast<const mrt::path::State*>(state);
    a.pending = static_cast<const float4*>(pending);
    a.shadowResults = static_cast<const int4*>(shadowResults);
    a.radiance = reinterpret_cast<float4*>(radiance);
    return launched(mrt::launch_path_accumulate(a, plan.grid, static_cast<hipStream_t>(stream)), "path accumulate launch");
}

int mrt_path_resolve(int32_t numSamples, int32_t firstPrimary, int32_t numPrimary, const int32_t* primarySlotToId,
                     const void* primaryResults, const float* radiance, uint32_t* pixels, float* image, void* stream) {
    const mrt::PathPlan plan = mrt::plan_path_resolve(numSamples, firstPrimary, numPrimary);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    if (plan.empty) return MRT_OK;
    if (!primarySlotToId || !primaryResults || !radiance || !pixels) return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(primaryResults) || !aligned16(radiance) || !aligned16(image))
        return fail(MRT_ERR_INVALID_ARG, "results, radiance or image not 16-byte aligned");
    mrt::PathResolveLaunch a{};
    a.numSamples = numSamples;
    a.firstPrimary = firstPrimary;
    a.numPrimary = numPrimary;
    a.primarySlotToId = primarySlotToId;
    a.primaryResults = static_cast<const int4*>(primaryResults);
    a.radiance = reinterpret_cast<const float4*>(radiance);
    a.pixels = pixels;
    a.image = reinterpret_cast<float4*>(image);
    return launched(mrt::launch_path_resolve(a, plan.grid, static_cast<hipStream_t>(stream)), "path resolve launch");
}

}  // extern "C"
