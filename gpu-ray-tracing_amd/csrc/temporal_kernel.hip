// temporal_kernel.hip — the temporal accumulation's kernels on the device (gfx950)
// (temporal_kernel.hpp). The C-ABI that calls them is temporal_api.cpp.
//
//   motion_kernel       one lane per primary slot: the slot's ray (two 16-byte loads) and result
//                       (one), the triangle's three indices and twice three vertices, one 16-byte
//                       store of the previous position
//   accumulate_kernel   one lane per pixel: the pixel's image, guide (two 16-byte loads) and albedo,
//                       its previous position where the geometry moved, then up to four taps of
//                       the previous frame's guide (32 bytes) and history (16) each, gathered
//                       through the caches: a tap's address depends on the reprojection, so nothing
//                       is staged in LDS. <Tiled> only changes which pixel a lane owns: 256
//                       consecutive pixels of the frame per workgroup (a wave is 64 consecutive
//                       pixels), or a 32 x 8 tile decoded from the one-dimensional block index as
//                       denoise_kernel.hip's filter_kernel does
//
// No workgroup waits on another and there are no atomics: a call reads the previous frame's buffers
// and writes this frame's. The per-pixel arithmetic is csrc/temporal_common.hpp, the same code the
// host runs (csrc/host/temporal.cpp); this file is built without denormal flushing (Makefile), so
// the bits are the host's.
#include "temporal_kernel.hpp"

#include "record_device.hpp"
#include "temporal_limits.hpp"

namespace mrt {
namespace {

using namespace temporal;

struct MotionArgs : TemporalMotionLaunch {};

__global__ __launch_bounds__(kThreads) void motion_kernel(MotionArgs a) {
    PrimarySlot s;
    if (!load_primary_slot((int)(blockIdx.x * kThreads + threadIdx.x), a.numPrimary, a.primarySlotToId, a.numPixels,
                           a.primaryRays, a.primaryResults, s))
        return;
    a.prevPosition[s.pixel] =
        as_float4(motion_one(s.ray, s.id, s.t, a.triangles, a.numTris, a.vertices, a.prevVertices, a.numVertices));
}

struct AccumulateArgs : TemporalAccumulateLaunch {};

struct GlobalSource {
    const AccumulateArgs& a;
    __device__ Color image(int p) const { return as_color(a.image[p]); }
    __device__ Guide guide(int p) const { return load_guide(a.guide, p); }
    __device__ Color albedo(int p) const { return as_color(a.albedo[p]); }
    __device__ Color prev_position(int p) const { return as_color(a.prevPosition[p]); }
    __device__ Guide prev_guide(int q) const { return load_guide(a.prevGuide, q); }
    __device__ Color prev_history(int q) const { return as_color(a.prevHistory[q]); }
};

template <bool Tiled>
__global__ __launch_bounds__(kThreads) void accumulate_kernel(AccumulateArgs a) {
    int p;
    if (Tiled) {
        const int tileY = (int)blockIdx.x / a.tilesX, tileX = (int)blockIdx.x - tileY * a.tilesX;
        const int x = tileX * kTileW + (int)(threadIdx.x % kTileW), y = tileY * kTileH + (int)(threadIdx.x / kTileW);
        if (x >= a.k.width || y >= a.k.height) return;
        p = y * a.k.width + x;
    } else {
        p = (int)(blockIdx.x * kThreads + threadIdx.x);   // < 2^26 + 256
        if (p >= a.k.width * a.k.height) return;
    }
    Color history, result;
    accumulate_pixel(GlobalSource{a}, a.k, p, history, result);
    a.history[p] = as_float4(history);
    if (a.imageOut) a.imageOut[p] = as_float4(result);
    if (a.pixels) a.pixels[p] = denoise::pixel_of(result);
}

}  // namespace

hipError_t launch_temporal_motion(const TemporalMotionLaunch& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(motion_kernel, dim3((unsigned)grid), dim3((unsigned)kThreads), 0, s, MotionArgs{a});
    return hipGetLastError();
}

hipError_t launch_temporal_accumulate(const TemporalAccumulateLaunch& a, int grid, bool tiled, hipStream_t s) {
    if (tiled) hipLaunchKernelGGL(accumulate_kernel<true>, dim3((unsigned)grid), dim3((unsigned)kThreads), 0, s, AccumulateArgs{a});
    else hipLaunchKernelGGL(accumulate_kernel<false>, dim3((unsigned)grid), dim3((unsigned)kThreads), 0, s, AccumulateArgs{a});
    return hipGetLastError();
}

}  // namespace mrt
