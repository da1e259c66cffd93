// light_kernel.hpp — launch interface between the C-ABI glue (light_api.cpp) and the gfx950 kernels
// of a shadow frame (light_kernel.hip): the shadow-ray generators and the lit reconstruction. Grids
// come from the plan (frame_plan.hpp); one function is one logical step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "frame_limits.hpp"
#include "raygen_common.hpp"

namespace mrt {

struct ShadowLaunch {
    const rg::RayRec* inRays;
    const int2* inResults;   // RayResult viewed as int2 pairs: slot 2*i = {id, t bits}
    int numInput;
    int numSamples;
    float light[3];
    float radius;
    uint32_t seed;
    rg::RayRec* outRays;
    int32_t* outIdToSlot;
    int32_t* outSlotToId;
};

struct ShadowBlocksLaunch {
    const rg::RayRec* inRays;
    const int2* inResults;
    int numInput;
    int numSamples;
    float light[3];
    float radius;
    int batchInputs;          // P: input rays per batch
    int blockRays;            // B
    int64_t totalRays;        // numInput * numSamples
    int64_t outRays;          // output rays of this launch
    const int32_t* blocks;
    rg::RayRec* out;
    uint32_t seeds[frame::kMaxBatchSeeds];
    const uint32_t* seedTable;   // non-null: one seed per batch of the frame there, seeds[] unused
};

struct ReconstructLitLaunch {
    int numRaysPerPrimary, firstPrimary, numPrimary;
    const int32_t* primarySlotToId;
    const rg::RayRec* primaryRays;
    const int4* primaryResults;
    const int32_t* batchIdToSlot;   // NULL: identity (the generators' layout)
    const int4* batchResults;
    const float* triNormals;
    const uint32_t* triMaterialColor;
    float light[3];
    uint32_t* pixels;
};

// numSamples > 1: one thread per output ray; else one per input ray (launch_ao's rule).
hipError_t launch_shadow(const ShadowLaunch& a, int grid, hipStream_t s);
// A list of blocks' shadow rays, one thread per output ray; the seed table is launch_seed_table's
// (raygen_kernel.hpp).
hipError_t launch_shadow_blocks(const ShadowBlocksLaunch& a, int grid, hipStream_t s);
// One thread per primary ray of the batch.
hipError_t launch_reconstruct_lit(const ReconstructLitLaunch& a, int grid, hipStream_t s);

}  // namespace mrt
