// light_kernel.hip — a shadow frame's kernels on the device (gfx950): the rays from traced points
// towards an area light, and the direct lighting reconstructed from their any-hit results
// (light_kernel.hpp). The C-ABI that calls them is light_api.cpp.
//
//   shadow_kernel           <- rayGenShadowKernel (reference RayGenKernels.cu:231-293)
//   shadow_blocks_kernel    the same rays for a list of blocks of a frame's ray order
//   reconstruct_lit_kernel  the share of a primary's shadow rays that reached the light, times the
//                           cosine at the surface and its material colour
//
// The per-ray arithmetic is csrc/light_common.hpp, the same code the host runs (csrc/host/light.cpp);
// this file is built without denormal flushing (Makefile), so the bits are the host's. These are
// streaming kernels of 256-thread workgroups. A generator lane reads its input ray (32 B) and
// result (8 B) once — the S lanes of one input ray share the cache lines — and writes its ray as
// two 16-byte stores, so a wave's stores cover 2 KB of consecutive 128-byte lines.
#include "light_kernel.hpp"

#include "light_common.hpp"
#include "record_device.hpp"

namespace mrt {
namespace {

using namespace frame;

struct InputRay {
    rg::RayRec ray;
    int32_t id;
    float t;
};

__device__ inline InputRay load_input(const rg::RayRec* rays, const int2* results, int p) {
    const rg::RayRec ray = load_ray(rays, p);
    const int2 res = results[2 * (int64_t)p];   // the result's first 8 of 16 bytes
    return InputRay{ray, res.x, __int_as_float(res.y)};
}

struct ShadowArgs : ShadowLaunch {};

// One thread per output ray; numSamples 1 makes that one per input ray.
__global__ __launch_bounds__(kThreads) void shadow_kernel(ShadowArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (int64_t)a.numInput * a.numSamples) return;
    const int task = (int)(gid / a.numSamples), i = (int)(gid - (int64_t)task * a.numSamples);
    const InputRay in = load_input(a.inRays, a.inResults, task);
    store_ray(a.outRays, gid,
              light::shadow_sample(in.ray, in.id, in.t, a.seed, (uint32_t)task, i, a.numSamples, a.light, a.radius));
    if (a.outIdToSlot) a.outIdToSlot[gid] = (int32_t)gid;
    if (a.outSlotToId) a.outSlotToId[gid] = (int32_t)gid;
}

// A frame's shadow rays in block order (mrt_raygen_shadow_blocks): raygen_kernel.hip's
// ao_blocks_kernel with this generator. Output ray j is ray g = blocks[j / B] * B + j % B of the
// frame's sequence g = p * S + i; batch k = p / P hashes seed_k + (p - k * P).
struct ShadowBlocksArgs : ShadowBlocksLaunch {};

template <bool kSeedTable>
__global__ __launch_bounds__(kThreads) void shadow_blocks_kernel(ShadowBlocksArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= a.outRays) return;
    const int64_t k = j / a.blockRays;
    const int64_t g = (int64_t)a.blocks[k] * a.blockRays + (j - k * a.blockRays);
    // past the frame's end: the (last-listed) partial block; a block id outside the frame writes nothing
    if (g < 0 || g >= a.totalRays) return;
    const int p = (int)(g / a.numSamples), i = (int)(g - (int64_t)p * a.numSamples);
    const int batch = p / a.batchInputs;   // < the frame's batches: p < numInput
    const uint32_t seed = kSeedTable ? a.seedTable[batch] : a.seeds[batch];
    const InputRay in = load_input(a.inRays, a.inResults, p);
    store_ray(a.out, j,
              light::shadow_sample(in.ray, in.id, in.t, seed, (uint32_t)(p - batch * a.batchInputs), i, a.numSamples,
                                   a.light, a.radius));
}

struct ReconstructLitArgs : ReconstructLitLaunch {};

// One thread per primary ray of the batch: count its n shadow rays that missed everything up to
// their light samples, weigh by the cosine at the surface and the material, write one ABGR pixel.
__global__ __launch_bounds__(kThreads) void reconstruct_lit_kernel(ReconstructLitArgs a) {
    const int task = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (task >= a.numPrimary) return;
    const int n = a.numRaysPerPrimary;
    const int primarySlot = a.firstPrimary + task;
    const int4 pr = a.primaryResults[primarySlot];
    const int pixel = a.primarySlotToId[primarySlot];
    if (pr.x == -1) {
        a.pixels[pixel] = light::background_pixel();
        return;
    }
    const int64_t base = (int64_t)task * n;
    int unblocked = 0;
    for (int i = 0; i < n; i++) {
        const int64_t slot = a.batchIdToSlot ? a.batchIdToSlot[base + i] : base + i;
        unblocked += a.batchResults[slot].x == -1;
    }
    const InputRay in = load_input(a.primaryRays, reinterpret_cast<const int2*>(a.primaryResults), primarySlot);
    const float k = light::lit_factor(in.ray, in.t, a.triNormals + 3 * (int64_t)pr.x, a.light);
    a.pixels[pixel] = light::lit_pixel(a.triMaterialColor[pr.x], k, unblocked, n);
}

template <class K, class A>
hipError_t launch(K kernel, int grid, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_shadow(const ShadowLaunch& a, int grid, hipStream_t s) {
    return launch(shadow_kernel, grid, s, ShadowArgs{a});
}

hipError_t launch_shadow_blocks(const ShadowBlocksLaunch& a, int grid, hipStream_t s) {
    if (a.seedTable) return launch(shadow_blocks_kernel<true>, grid, s, ShadowBlocksArgs{a});
    return launch(shadow_blocks_kernel<false>, grid, s, ShadowBlocksArgs{a});
}

hipError_t launch_reconstruct_lit(const ReconstructLitLaunch& a, int grid, hipStream_t s) {
    return launch(reconstruct_lit_kernel, grid, s, ReconstructLitArgs{a});
}

}  // namespace mrt
