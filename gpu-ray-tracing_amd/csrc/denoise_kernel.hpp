// denoise_kernel.hpp — launch interface between the C-ABI glue (denoise_api.cpp) and the gfx950
// kernels of the denoiser (denoise_kernel.hip): the features of a traced primary batch, one
// iteration of the filter with its taps loaded directly or staged in LDS, and the iteration-free
// modulate pass. Grids come from the plan
// (denoise_plan.hpp); one function is one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "denoise_common.hpp"

namespace mrt {

struct DenoiseFeaturesLaunch {
    int32_t numPrimary, numPixels;
    int64_t numTris;
    const int32_t* primarySlotToId;
    const rg::RayRec* primaryRays;
    const int4* primaryResults;
    const float* triNormals;
    const uint32_t* triMaterialColor;
    float4* guide;    // two per pixel
    float4* albedo;
};

struct DenoiseFilterLaunch {
    int32_t width, height, tilesX;
    int32_t residues;        // staged only (DenoiseLaunchPlan)
    int32_t step, squarings;
    float invPlane, invColor2;
    int32_t first, last;     // first: `in` is the frame's image and is demodulated as it is loaded;
                             // last: the result is remodulated and goes to imageOut / pixels
    const float4* in;
    const float4* guide;
    const float4* albedo;
    float4* out;             // !last: the next iteration's colours; last: imageOut, may be NULL
    uint32_t* pixels;        // last only, may be NULL
};

// One thread per primary slot.
hipError_t launch_denoise_features(const DenoiseFeaturesLaunch& a, int grid, hipStream_t s);
// One thread per pixel, tilesX * tilesY workgroups of one tile each, every tap a global load.
hipError_t launch_denoise_filter(const DenoiseFilterLaunch& a, int grid, hipStream_t s);
// The same iteration with the tile's taps staged in ldsBytes of LDS (steps up to denoise::kTiledMaxStep).
hipError_t launch_denoise_filter_tiled(const DenoiseFilterLaunch& a, int grid, int ldsBytes, hipStream_t s);
// iterations == 0: demodulate, remodulate and write, the same grid.
hipError_t launch_denoise_modulate(const DenoiseFilterLaunch& a, int grid, hipStream_t s);

}  // namespace mrt
