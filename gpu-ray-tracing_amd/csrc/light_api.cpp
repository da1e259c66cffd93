// light_api.cpp — the C-ABI of a shadow frame's steps around its trace: mrt_raygen_shadow /
// _shadow_blocks and mrt_reconstruct_lit. Per export: the argument checks, the plan
// (frame_plan.cpp: counts, grids), the launches (light_kernel.hip). Everything is enqueued on the
// caller's stream; nothing waits on the host and no state outlives a call.
//
//   mrt_raygen_shadow  <- RayGen::shadow (reference RayGen.cc:147-183, commented out there)
#include <cstdint>

#include "api_checks.hpp"
#include "api_common.hpp"
#include "frame_plan.hpp"
#include "light_kernel.hpp"
#include "raygen_kernel.hpp"   // launch_seed_table

using mrt::aligned16;   // rays are read and written as 16-byte halves
using mrt::fail;
using mrt::hipFail;
using mrt::launched;

extern "C" {

int mrt_raygen_shadow(const void* inRays, const void* inResults, int32_t numInputRays, int32_t numSamples,
                      const float light[3], float lightRadius, uint32_t seed, void* outRays, int32_t* outIdToSlot,
                      int32_t* outSlotToId, void* stream) {
    if (numInputRays < 0 || numSamples < 1) return fail(MRT_ERR_INVALID_ARG, "bad ray/sample count");
    if (numInputRays == 0) return MRT_OK;
    if (!inRays || !inResults || !outRays || !light) return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(inRays) || !aligned16(outRays)) return fail(MRT_ERR_INVALID_ARG, "rays not 16-byte aligned");
    const int64_t total = (int64_t)numInputRays * numSamples;
    if (total > INT32_MAX) return fail(MRT_ERR_TOO_LARGE, "too many output rays");
    mrt::ShadowLaunch a{};
    a.inRays = static_cast<const mrt::rg::RayRec*>(inRays);
    a.inResults = static_cast<const int2*>(inResults);
    a.numInput = numInputRays;
    a.numSamples = numSamples;
    for (int k = 0; k < 3; k++) a.light[k] = light[k];
    a.radius = lightRadius;
    a.seed = seed;
    a.outRays = static_cast<mrt::rg::RayRec*>(outRays);
    a.outIdToSlot = outIdToSlot;
    a.outSlotToId = outSlotToId;
    return launched(mrt::launch_shadow(a, mrt::grid_1d(total), static_cast<hipStream_t>(stream)), "raygen shadow launch");
}

int mrt_raygen_shadow_blocks(const void* inRays, const void* inResults, int32_t numInputRays, int32_t numSamples,
                             const float light[3], float lightRadius, const uint32_t* batchSeeds, int32_t numBatches,
                             int32_t batchInputRays, const int32_t* blocks, int32_t numBlocks, int32_t blockRays,
                             int64_t numOutRays, void* outRays, void* stream) {
    const mrt::AOBlocksPlan p =
        mrt::plan_ao_blocks(numInputRays, numSamples, numBatches, batchInputRays, numBlocks, blockRays, numOutRays);
    if (p.rc != MRT_OK) return fail(p.rc, p.why);
    if (p.empty) return MRT_OK;
    if (!inRays || !inResults || !outRays || !blocks || !batchSeeds || !light)
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(inRays) || !aligned16(outRays)) return fail(MRT_ERR_INVALID_ARG, "rays not 16-byte aligned");
    mrt::ShadowBlocksLaunch a{};
    a.inRays = static_cast<const mrt::rg::RayRec*>(inRays);
    a.inResults = static_cast<const int2*>(inResults);
    a.numInput = numInputRays;
    a.numSamples = numSamples;
    for (int k = 0; k < 3; k++) a.light[k] = light[k];
    a.radius = lightRadius;
    a.batchInputs = batchInputRays;
    a.blockRays = blockRays;
    a.totalRays = p.total;
    a.outRays = numOutRays;
    a.blocks = blocks;
    a.out = static_cast<mrt::rg::RayRec*>(outRays);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = mrt::grid_1d(numOutRays);   // one thread per output ray (the plan's grid is the AO kernels')
    if (p.seedsInArgs) {
        for (int64_t k = 0; k < p.needBatches; k++) a.seeds[k] = batchSeeds[k];
        return launched(mrt::launch_shadow_blocks(a, grid, s), "raygen shadow blocks launch");
    }
    // More batches than the arguments hold: the seeds go to stream-ordered scratch, as in
    // mrt_raygen_ao_blocks.
    mrt::StreamScratch table;
    if (hipError_t e = table.alloc((size_t)p.needBatches * sizeof(uint32_t), s)) return hipFail(e, "hipMallocAsync(batch seeds)");
    a.seedTable = table.as<uint32_t>();
    hipError_t e = mrt::launch_seed_table(table.as<uint32_t>(), batchSeeds, p.needBatches, s);
    if (e == hipSuccess) e = mrt::launch_shadow_blocks(a, grid, s);
    return launched(e, "raygen shadow blocks launch", table, "hipFreeAsync(batch seeds)");
}

int mrt_reconstruct_lit(int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                        const int32_t* primarySlotToId, const void* primaryRays, const void* primaryResults,
                        const int32_t* batchIdToSlot, const void* batchResults, const float* triNormals,
                        const uint32_t* triMaterialColor, const float light[3], uint32_t* pixels, void* stream) {
    if (numRaysPerPrimary < 1 || firstPrimary < 0 || numPrimary < 0) return fail(MRT_ERR_INVALID_ARG, "bad batch shape");
    if ((int64_t)numPrimary * numRaysPerPrimary > INT32_MAX || (int64_t)firstPrimary + numPrimary > INT32_MAX)
        return fail(MRT_ERR_TOO_LARGE, "too many rays");
    if (numPrimary == 0) return MRT_OK;
    if (!primarySlotToId || !primaryRays || !primaryResults || !batchResults || !triNormals || !triMaterialColor ||
        !light || !pixels)
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (!aligned16(primaryRays)) return fail(MRT_ERR_INVALID_ARG, "rays not 16-byte aligned");
    mrt::ReconstructLitLaunch a{};
    a.numRaysPerPrimary = numRaysPerPrimary;
    a.firstPrimary = firstPrimary;
    a.numPrimary = numPrimary;
    a.primarySlotToId = primarySlotToId;
    a.primaryRays = static_cast<const mrt::rg::RayRec*>(primaryRays);
    a.primaryResults = static_cast<const int4*>(primaryResults);
    a.batchIdToSlot = batchIdToSlot;
    a.batchResults = static_cast<const int4*>(batchResults);
    a.triNormals = triNormals;
    a.triMaterialColor = triMaterialColor;
    for (int k = 0; k < 3; k++) a.light[k] = light[k];
    a.pixels = pixels;
    return launched(mrt::launch_reconstruct_lit(a, mrt::grid_1d(numPrimary), static_cast<hipStream_t>(stream)),
                    "reconstruct lit launch");
}

}  // extern "C"
