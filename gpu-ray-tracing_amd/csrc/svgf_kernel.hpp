// svgf_kernel.hpp — launch interface between the C-ABI glue (svgf_api.cpp) and the gfx950 kernels of
// the variance-guided filter (svgf_kernel.hip): the accumulation with moments in its two launch
// shapes, the variance launch, and one iteration with its taps loaded directly or staged in LDS.
// Grids come from the plans (temporal_plan.hpp, svgf_plan.hpp); one function is one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "svgf_common.hpp"
#include "temporal_kernel.hpp"

namespace mrt {

struct SvgfAccumulateLaunch : TemporalAccumulateLaunch {
    const float4* prevMoments;   // not read where !k.havePrev
    float4* moments;
};

struct SvgfFilterLaunch {
    int32_t width, height, tilesX;
    int32_t residues;        // staged only (SvgfLaunchPlan)
    int32_t step, squarings;
    float invPlane, sigmaLum2;
    int32_t last;            // the result is remodulated and goes to imageOut / pixels / varianceOut
    const float4* in;        // the variance launch: unused; an iteration: c_k
    const float4* image;     // the accumulated frame: the variance launch's input, the last launch's w
    const float4* guide;
    const float4* albedo;
    const float4* moments;   // the variance launch only
    float4* out;             // !last: c_{k+1}; last: imageOut, may be NULL
    uint32_t* pixels;        // last only, may be NULL
    float* varianceOut;      // last only, may be NULL
};

// One thread per pixel: 256 consecutive pixels per workgroup, or (tiled) one 32 x 8 tile.
hipError_t launch_svgf_accumulate(const SvgfAccumulateLaunch& a, int grid, bool tiled, hipStream_t s);
// One thread per pixel of a 32 x 8 tile: c_0 from the accumulated frame and its moments.
hipError_t launch_svgf_variance(const SvgfFilterLaunch& a, int grid, hipStream_t s);
// One thread per pixel, tilesX * tilesY workgroups of one tile each, every tap a global load.
hipError_t launch_svgf_iterate(const SvgfFilterLaunch& a, int grid, hipStream_t s);
// The same iteration with the tile's taps staged in ldsBytes of LDS (steps up to svgf::kTiledMaxStep).
hipError_t launch_svgf_iterate_tiled(const SvgfFilterLaunch& a, int grid, int ldsBytes, hipStream_t s);

}  // namespace mrt
