// temporal_plan.hpp — what the temporal accumulation's C-ABI (temporal_api.cpp) and its host
// statements (host/temporal.cpp) decide before they touch anything: the scalar checks and limits of
// a call, 1 / sigmaPlane, the launch shape and the grid. Plain C++ with no HIP in it (the host
// compiler builds temporal_plan.cpp), so tests/cpp/temporal_driver.cpp runs it on the CPU.
#pragma once
#include <cstdint>

#include "temporal_limits.hpp"

namespace mrt {

struct TemporalPlan {
    int rc;            // MRT_OK, or the error the call returns before it touches anything
    const char* why;
    bool empty;        // motion only: no slot or no pixel: MRT_OK, nothing launched
    int grid;          // workgroups of temporal::kThreads lanes
    int tiled;         // accumulate only: 32 x 8 tiles, else 256 consecutive pixels per workgroup
    int tilesX, tilesY;   // tiled only
    float invPlane;    // accumulate only: 1 / sigmaPlane
};

// Checks, in this order: a negative count (MRT_ERR_INVALID_ARG); more than 2^26 slots or pixels
// (MRT_ERR_TOO_LARGE); then empty.
TemporalPlan plan_temporal_motion(int32_t numPrimary, int64_t numTris, int64_t numVertices, int32_t numPixels);
// Checks, in this order: width or height < 1, maxHistory < 1, a variant outside 0..2, a sigmaPlane
// that is not above 0, a NaN normalCos (MRT_ERR_INVALID_ARG); more than 2^26 pixels, maxHistory above
// 2^20 (MRT_ERR_TOO_LARGE). variant: 0 = the shipped shape (temporal::kDefaultTiled), 1 = linear, 2 = tiled.
TemporalPlan plan_temporal_accumulate(int32_t width, int32_t height, int32_t maxHistory, float normalCos, float sigmaPlane,
                                      int32_t variant);

}  // namespace mrt
