// light.cpp — an area light's shadow rays and the lit reconstruction on the CPU: the statements
// mrt_raygen_shadow / _shadow_blocks and mrt_reconstruct_lit (csrc/light_kernel.hip) are checked
// against, term for term (csrc/light_common.hpp).
#include <cstring>

#include "../../../include/mrt_host.h"
#include "../light_common.hpp"
#include "host_error.hpp"

namespace mrt {
namespace {

struct Result {   // RayResult (reference Util.hh:78-89)
    int32_t id;
    float t;
    int32_t pad[2];
};
static_assert(sizeof(Result) == 16 && sizeof(rg::RayRec) == 32, "the reference's record sizes");

}  // namespace

void gen_shadow_rays(const void* inRays, const void* inResults, int64_t numInput, int numSamples, const float light[3],
                     float radius, uint32_t seed, void* outRays) {
    const char* rays = static_cast<const char*>(inRays);
    const char* results = static_cast<const char*>(inResults);
    char* out = static_cast<char*>(outRays);
    for (int64_t task = 0; task < numInput; task++) {
        rg::RayRec in;
        Result res;
        std::memcpy(&in, rays + 32 * task, 32);
        std::memcpy(&res, results + 16 * task, 16);
        float origin[3], offset[3];
        light::shadow_origin(in, res.t, origin);
        light::shadow_offset(seed, (uint32_t)task, offset);
        for (int i = 0; i < numSamples; i++) {
            const rg::RayRec r = light::shadow_ray(origin, offset, res.id, i, numSamples, light, radius);
            std::memcpy(out + 32 * (task * numSamples + i), &r, 32);
        }
    }
}

void reconstruct_lit(int n, int firstPrimary, int numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                     const void* primaryResults, const int32_t* batchIdToSlot, const void* batchResults,
                     const float* triNormals, const uint32_t* triMaterialColor, const float light[3], uint32_t* pixels) {
    const char* rays = static_cast<const char*>(primaryRays);
    const char* pres = static_cast<const char*>(primaryResults);
    const char* bres = static_cast<const char*>(batchResults);
    for (int64_t task = 0; task < numPrimary; task++) {
        const int64_t slot = firstPrimary + task;
        rg::RayRec in;
        Result res;
        std::memcpy(&in, rays + 32 * slot, 32);
        std::memcpy(&res, pres + 16 * slot, 16);
        uint32_t& pixel = pixels[primarySlotToId[slot]];
        if (res.id == -1) {
            pixel = light::background_pixel();
            continue;
        }
        int unblocked = 0;
        for (int i = 0; i < n; i++) {
            const int64_t at = batchIdToSlot ? batchIdToSlot[task * n + i] : task * n + i;
            int32_t id;
            std::memcpy(&id, bres + 16 * at, 4);
            unblocked += id == -1;
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
