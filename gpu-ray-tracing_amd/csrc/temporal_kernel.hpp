// temporal_kernel.hpp — launch interface between the C-ABI glue (temporal_api.cpp) and the gfx950
// kernels of the temporal accumulation (temporal_kernel.hip): the previous position of a traced
// primary batch's hits, and the accumulation of a frame in its two launch shapes. Grids come from
// the plan (temporal_plan.hpp); one function is one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "temporal_common.hpp"

namespace mrt {

struct TemporalMotionLaunch {
    int32_t numPrimary, numPixels;
    int64_t numTris, numVertices;
    const int32_t* primarySlotToId;
    const rg::RayRec* primaryRays;
    const int4* primaryResults;
    const int32_t* triangles;
    const float* vertices;
    const float* prevVertices;
    float4* prevPosition;
};

struct TemporalAccumulateLaunch {
    temporal::Constants k;
    int32_t tilesX;              // tiled only
    const float4* image;
    const float4* guide;         // two per pixel
    const float4* albedo;
    const float4* prevPosition;  // NULL where !k.hasPrevPosition
    const float4* prevGuide;     // not read where !k.havePrev
    const float4* prevHistory;
    float4* history;
    float4* imageOut;            // may be NULL
    uint32_t* pixels;            // may be NULL
};

// One thread per primary slot.
hipError_t launch_temporal_motion(const TemporalMotionLaunch& a, int grid, hipStream_t s);
// One thread per pixel: 256 consecutive pixels per workgroup, or (tiled) one 32 x 8 tile.
hipError_t launch_temporal_accumulate(const TemporalAccumulateLaunch& a, int grid, bool tiled, hipStream_t s);

}  // namespace mrt
