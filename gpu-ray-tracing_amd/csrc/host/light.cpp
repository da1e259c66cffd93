// light.cpp — an area light's shadow rays and the lit reconstruction on the CPU: the statements
// mrt_raygen_shadow / _shadow_blocks and mrt_reconstruct_lit (csrc/light_kernel.hip) are checked
// against, term for term (csrc/light_common.hpp).
#include "../../../include/mrt_host.h"
#include "../light_common.hpp"
#include "host_error.hpp"
#include "records.hpp"

namespace mrt {

static_assert(sizeof(rg::RayRec) == 32, "the reference's record size");

void gen_shadow_rays(const void* inRays, const void* inResults, int64_t numInput, int numSamples, const float light[3],
                     float radius, uint32_t seed, void* outRays) {
    for (int64_t task = 0; task < numInput; task++) {
        const rg::RayRec in = get_record<rg::RayRec>(inRays, task);
        const RayResult res = get_record<RayResult>(inResults, task);
        float origin[3], offset[3];
        light::shadow_origin(in, res.t, origin);
        light::shadow_offset(seed, (uint32_t)task, offset);
        for (int i = 0; i < numSamples; i++) {
            put_record(outRays, task * numSamples + i, light::shadow_ray(origin, offset, res.id, i, numSamples, light, radius));
        }
    }
}

void reconstruct_lit(int n, int firstPrimary, int numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                     const void* primaryResults, const int32_t* batchIdToSlot, const void* batchResults,
                     const float* triNormals, const uint32_t* triMaterialColor, const float light[3], uint32_t* pixels) {
    for (int64_t task = 0; task < numPrimary; task++) {
        const int64_t slot = firstPrimary + task;
        const rg::RayRec in = get_record<rg::RayRec>(primaryRays, slot);
        const RayResult res = get_record<RayResult>(primaryResults, slot);
        uint32_t& pixel = pixels[primarySlotToId[slot]];
        if (res.id == -1) {
            pixel = light::background_pixel();
            continue;
        }
        int unblocked = 0;
        for (int i = 0; i < n; i++) {
            const int64_t at = batchIdToSlot ? batchIdToSlot[task * n + i] : task * n + i;
            unblocked += get_record<RayResult>(batchResults, at).id == -1;
        }
        const float k = light::lit_factor(in, res.t, triNormals + 3 * (int64_t)res.id, light);
        pixel = light::lit_pixel(triMaterialColor[res.id], k, unblocked, n);
    }
}

}  // namespace mrt

extern "C" {

int mrth_shadow_rays(const void* inRays, const void* inResults, int64_t numInputRays, int32_t numSamples,
                     const float light[3], float lightRadius, uint32_t seed, void* outRays) {
    if (numInputRays < 0 || numSamples < 1) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "shadow_rays: bad ray/sample count");
    if (numInputRays == 0) return MRTH_OK;
    if (!inRays || !inResults || !light || !outRays) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "shadow_rays: null argument");
    if (numInputRays * numSamples > INT32_MAX) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "shadow_rays: too many output rays");
    mrt::gen_shadow_rays(inRays, inResults, numInputRays, numSamples, light, lightRadius, seed, outRays);
    return MRTH_OK;
}

int mrth_reconstruct_lit(int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                         const int32_t* primarySlotToId, const void* primaryRays, const void* primaryResults,
                         const int32_t* batchIdToSlot, const void* batchResults, const float* triNormals,
                         const uint32_t* triMaterialColor, const float light[3], uint32_t* pixels) {
    if (numRaysPerPrimary < 1 || firstPrimary < 0 || numPrimary < 0 ||
        (int64_t)numPrimary * numRaysPerPrimary > INT32_MAX || (int64_t)firstPrimary + numPrimary > INT32_MAX)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "reconstruct_lit: bad batch shape");
    if (numPrimary == 0) return MRTH_OK;
    if (!primarySlotToId || !primaryRays || !primaryResults || !batchResults || !triNormals || !triMaterialColor ||
        !light || !pixels)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "reconstruct_lit: null argument");
    mrt::reconstruct_lit(numRaysPerPrimary, firstPrimary, numPrimary, primarySlotToId, primaryRays, primaryResults,
                         batchIdToSlot, batchResults, triNormals, triMaterialColor, light, pixels);
    return MRTH_OK;
}

}  // extern "C"
