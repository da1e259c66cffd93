// denoise_api.cpp — the C-ABI of the path frame's denoiser: mrt_denoise_features and
// mrt_denoise_filter. Per export: the plan (denoise_plan.cpp: scalar checks, limits, constants,
// grids), the pointer checks, the launches (denoise_kernel.hip). Everything is enqueued on the
// caller's stream; nothing waits on the host, nothing is allocated and no state outlives a call.
#include <cstdint>

#include "api_checks.hpp"
#include "api_common.hpp"
#include "denoise_kernel.hpp"
#include "denoise_plan.hpp"

using mrt::aligned16;
using mrt::any_overlap;
using mrt::fail;
using mrt::launched;
using mrt::Span;

extern "C" {

int mrt_denoise_features(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                         const void* primaryResults, const float* triNormals, const uint32_t* triMaterialColor,
                         int64_t numTris, int32_t numPixels, void* guide, float* albedo, void* stream) {
    const mrt::DenoisePlan plan = mrt::plan_denoise_features(numPrimary, numTris, numPixels);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    if (plan.empty) return MRT_OK;
    if (!primarySlotToId || !primaryRays || !primaryResults || !guide || !albedo || (numTris > 0 && (!triNormals || !triMaterialColor)))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(primaryRays) || !aligned16(primaryResults) || !aligned16(guide) || !aligned16(albedo))
        return fail(MRT_ERR_INVALID_ARG, "rays, results, guide or albedo not 16-byte aligned");
    const int64_t n = numPrimary, px = numPixels;
    const Span ins[] = {{primarySlotToId, 4 * n}, {primaryRays, 32 * n}, {primaryResults, 16 * n},
                        {triNormals, 12 * numTris}, {triMaterialColor, 4 * numTris}};
    const Span outs[] = {{guide, 32 * px}, {albedo, 16 * px}};
    if (any_overlap(ins, outs)) return fail(MRT_ERR_INVALID_ARG, "an output buffer overlaps an input or another output");
    mrt::DenoiseFeaturesLaunch a{};
    a.numPrimary = numPrimary;
    a.numPixels = numPixels;
    a.numTris = numTris;
    a.primarySlotToId = primarySlotToId;
    a.primaryRays = static_cast<const mrt::rg::RayRec*>(primaryRays);
    a.primaryResults = static_cast<const int4*>(primaryResults);
    a.triNormals = triNormals;
    a.triMaterialColor = triMaterialColor;
    a.guide = static_cast<float4*>(guide);
    a.albedo = reinterpret_cast<float4*>(albedo);
    const hipError_t e = mrt::launch_denoise_features(a, plan.grid, static_cast<hipStream_t>(stream));
    return launched(e, "denoise features launch");
}

int mrt_denoise_filter(const mrt_denoise_params* q, void* stream) {
    if (!q) return fail(MRT_ERR_INVALID_ARG, "null params");
    const mrt::DenoisePlan plan =
        mrt::plan_denoise_filter(q->width, q->height, q->iterations, q->normalSquarings, q->sigmaColor, q->sigmaPlane, q->variant);
    if (plan.rc != MRT_OK) return fail(plan.rc, plan.why);
    const int N = q->iterations;
    float* const scratch0 = N >= 2 ? q->scratch[0] : nullptr;   // an iteration count that does not use one
    float* const scratch1 = N >= 3 ? q->scratch[1] : nullptr;   // ignores it
    if (!q->image || !q->guide || !q->albedo || (N >= 2 && !scratch0) || (N >= 3 && !scratch1))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!q->imageOut && !q->pixels) return fail(MRT_ERR_INVALID_ARG, "neither imageOut nor pixels");
    if (!aligned16(q->image) || !aligned16(q->guide) || !aligned16(q->albedo) || !aligned16(scratch0) ||
        !aligned16(scratch1) || !aligned16(q->imageOut))
        return fail(MRT_ERR_INVALID_ARG, "image, guide, albedo, scratch or imageOut not 16-byte aligned");
    const int64_t px = (int64_t)q->width * q->height;
    const Span ins[] = {{q->image, 16 * px}, {q->guide, 32 * px}, {q->albedo, 16 * px}};
    const Span outs[] = {{scratch0, 16 * px}, {scratch1, 16 * px}, {q->imageOut, 16 * px}, {q->pixels, 4 * px}};
    if (any_overlap(ins, outs)) return fail(MRT_ERR_INVALID_ARG, "an output or scratch buffer overlaps an input or another output");
    mrt::DenoiseFilterLaunch a{};
    a.width = q->width;
    a.height = q->height;
    a.squarings = q->normalSquarings;
    a.invPlane = plan.invPlane;
    a.guide = static_cast<const float4*>(q->guide);
    a.albedo = reinterpret_cast<const float4*>(q->albedo);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* const pingpong[2] = {scratch0, scratch1};
    const float* in = q->image;
    hipError_t e = hipSuccess;
    for (int k = 0; k < plan.launches && e == hipSuccess; k++) {
        a.first = k == 0;
        a.last = k == plan.launches - 1;
        const mrt::DenoiseLaunchPlan& it = plan.at[k];
        a.step = it.step;
        a.tilesX = it.tilesX;
        a.residues = it.residues;
        a.invColor2 = it.invColor2;
        a.in = reinterpret_cast<const float4*>(in);
        a.out = reinterpret_cast<float4*>(a.last ? q->imageOut : pingpong[k & 1]);
        a.pixels = a.last ? q->pixels : nullptr;
        if (N == 0) e = mrt::launch_denoise_modulate(a, it.grid, s);
        else if (it.tiled) e = mrt::launch_denoise_filter_tiled(a, it.grid, it.ldsBytes, s);
        else e = mrt::launch_denoise_filter(a, it.grid, s);
        in = pingpong[k & 1];
    }
    return launched(e, "denoise filter launch");
}

}  // extern "C"
