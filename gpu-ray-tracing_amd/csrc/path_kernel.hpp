// path_kernel.hpp — launch interface between the C-ABI glue (path_api.cpp) and the gfx950 kernels
// of a path frame (path_kernel.hip): the survivor count, its scan, the vertex step that places
// each survivor, the accumulation of a traced shadow batch and the resolve. Grids come from the
// plan (path_plan.hpp); one function is one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "path_common.hpp"

namespace mrt {

struct PathExtendLaunch {
    path::Params p;
    int32_t numSlots;
    int32_t numPaths;              // entries of radiance: a task outside [0, numPaths) is no path
    int32_t compact;
    const rg::RayRec* inRays;      // vertex 0: the batch's input rays, slot / S; else one per slot
    const int2* inResults;         // RayResult viewed as int2 pairs: entry 2*i = {id, t bits}
    const path::State* inState;    // vertex 0: unused
    rg::RayRec* outShadow;
    float4* outPending;
    rg::RayRec* outRays;           // unused at vertex == depth
    path::State* outState;
    float4* radiance;
    int32_t* counts;               // scratch: one entry per workgroup of the extend grid
    int32_t* liveCount;
};

struct PathAccumulateLaunch {
    int32_t numSlots;
    int32_t numPaths;
    const path::State* state;
    const float4* pending;
    const int4* shadowResults;
    float4* radiance;
};

struct PathResolveLaunch {
    int32_t numSamples, firstPrimary, numPrimary;
    const int32_t* primarySlotToId;
    const int4* primaryResults;
    const float4* radiance;
    uint32_t* pixels;
    float4* image;   // may be NULL
};

// One thread per slot: counts[workgroup] = its survivors.
hipError_t launch_path_count(const PathExtendLaunch& a, int grid, hipStream_t s);
// One workgroup: counts[] becomes its exclusive prefix sum, *liveCount the total.
hipError_t launch_path_scan(int32_t* counts, int numCounts, int32_t* liveCount, hipStream_t s);
// One thread per slot, the count's grid.
hipError_t launch_path_extend(const PathExtendLaunch& a, int grid, hipStream_t s);
hipError_t launch_path_accumulate(const PathAccumulateLaunch& a, int grid, hipStream_t s);
// One thread per primary ray of the batch.
hipError_t launch_path_resolve(const PathResolveLaunch& a, int grid, hipStream_t s);

}  // namespace mrt
