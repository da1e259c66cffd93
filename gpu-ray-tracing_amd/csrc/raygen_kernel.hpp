// raygen_kernel.hpp — launch interface between the C-ABI glue (frame_api.cpp) and the gfx950
// kernels around a frame's traces (raygen_kernel.hip): ray generation, the hit count and the
// reconstruction. Grids come from the plan (frame_plan.hpp); one function is one logical step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "frame_limits.hpp"
#include "raygen_common.hpp"

namespace mrt {

struct PrimaryLaunch {
    float m[16];   // column-major nscreen-to-world
    float ox, oy, oz, maxDist;
    float jx, jy;   // sample position inside the pixel
    int w, h;
    const int32_t* indexToPixel;
    rg::RayRec* rays;
    int32_t* slotToId;
    int32_t* idToSlot;
};

struct AOLaunch {
    const rg::RayRec* inRays;
    const int2* inResults;   // RayResult viewed as int2 pairs: slot 2*i = {id, t bits}
    int numInput;
    const float* normals;
    int64_t numTris;
    int numSamples;
    float maxDist;
    uint32_t seed;
    rg::RayRec* outRays;
    int32_t* outIdToSlot;
    int32_t* outSlotToId;
};

struct AOBlocksLaunch {
    const rg::RayRec* inRays;
    const int2* inResults;
    int numInput;
    const float* normals;
    int64_t numTris;
    int numSamples;
    float maxDist;
    int batchInputs;          // P: input rays per batch
    int blockRays;            // B
    int64_t totalRays;        // numInput * numSamples
    int64_t outRays;          // output rays of this launch
    const int32_t* blocks;
    rg::RayRec* out;
    uint32_t seeds[frame::kMaxBatchSeeds];
    const uint32_t* seedTable;   // non-null: one seed per batch of the frame there, seeds[] unused
};

struct ReconstructLaunch {
    int numRaysPerPrimary, firstPrimary, numPrimary, rayType;
    const int32_t* primarySlotToId;
    const int4* primaryResults;
    const int32_t* batchIdToSlot;   // NULL: identity (the device/host generators' layout)
    const int4* batchResults;
    const uint32_t* triMaterialColor;
    const uint32_t* triShadedColor;
    uint32_t* pixels;
};

// One thread per pixel of the w * h image.
hipError_t launch_primary(const PrimaryLaunch& a, int grid, hipStream_t s);
// numSamples > 1: one thread per output ray; else one per input ray.
hipError_t launch_ao(const AOLaunch& a, int grid, hipStream_t s);
// table[0, count) = seeds[0, count), through launches that carry kMaxBatchSeeds seeds each in
// their arguments (copied at launch: the caller's array is free on return; no host sync).
hipError_t launch_seed_table(uint32_t* table, const uint32_t* seeds, int64_t count, hipStream_t s);
// A list of blocks' secondary rays; tiled / grid: AOBlocksPlan's.
hipError_t launch_ao_blocks(const AOBlocksLaunch& a, bool tiled, int grid, hipStream_t s);
// *hitCount = results with id >= 0 among n: `blocks` partials of perBlock results each into
// partial[blocks], then their sum by one workgroup (blocks 0: *hitCount = 0).
hipError_t launch_count_hits(const int4* results, int n, int perBlock, int blocks, int32_t* partial, int32_t* hitCount,
                             hipStream_t s);
// One thread per primary ray of the batch: the tiled kernel for identity-layout AO/diffuse batches.
hipError_t launch_reconstruct(const ReconstructLaunch& a, int grid, hipStream_t s);

}  // namespace mrt
