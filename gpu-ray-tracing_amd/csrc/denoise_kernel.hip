// denoise_kernel.hip — the denoiser's kernels on the device (gfx950) (denoise_kernel.hpp). The C-ABI
// that calls them is denoise_api.cpp.
//
//   features_kernel   one lane per primary slot: the pixel's guide record (two 16-byte stores) and
//                     albedo (one) from the slot's ray (two 16-byte loads), result (one) and the
//                     triangle tables
//   filter_kernel     one iteration of the a-trous filter, one lane per pixel of a 32 x 8 tile, every
//                     tap loaded through the caches: a wave covers two 32-pixel rows, so each of the
//                     25 taps is two runs of 32 consecutive records per wave at every step. <First>
//                     demodulates the frame's image as it loads it, <Last> remodulates and writes
//                     imageOut and the pixels
//   filter_tiled_kernel   the same iteration with the taps staged in LDS. A workgroup owns 64
//                     consecutive columns of 4 rows `step` apart (one residue of y mod step), a wave
//                     per row. It stages the 8 rows of that residue its taps reach, 64 + 4 * step
//                     columns each (2 * step of halo per side), as three planes of 16-byte words
//                     (guide low, guide high, colour): rows are loaded coalesced, a pixel outside
//                     the frame is staged as a miss, and a wave reads each tap as 64 consecutive
//                     16-byte words of one plane. The footprint is 8 * (64 + 4 * step) records for
//                     256 pixels: 2.1x at step 1, 4x at step 16 (48 KB), against the direct
//                     kernel's 25 loads per pixel
//   modulate_kernel   iterations == 0: demodulate, remodulate, write
//
// Which of the two filter kernels runs at which step is the plan's choice (denoise_plan.cpp; the
// measurements: DESIGN §16); both run csrc/denoise_common.hpp's filter_pixel over another tap
// source, so their bits are equal. No workgroup waits on another and there are no float atomics: an iteration reads
// one image and writes another, and the iteration boundary is the launch boundary. The per-pixel
// arithmetic is csrc/denoise_common.hpp, the same code the host runs (csrc/host/denoise.cpp); this
// file is built without denormal flushing (Makefile), so the bits are the host's.
#include "denoise_kernel.hpp"

#include "denoise_limits.hpp"
#include "record_device.hpp"

namespace mrt {
namespace {

using namespace denoise;

struct FeaturesArgs : DenoiseFeaturesLaunch {};

__global__ __launch_bounds__(kThreads) void features_kernel(FeaturesArgs a) {
    PrimarySlot s;
    if (!load_primary_slot((int)(blockIdx.x * kThreads + threadIdx.x), a.numPrimary, a.primarySlotToId, a.numPixels,
                           a.primaryRays, a.primaryResults, s))
        return;
    Guide g;
    Color albedo;
    features_one(s.ray, s.id, s.t, a.triNormals, a.triMaterialColor, a.numTris, g, albedo);
    a.guide[2 * (int64_t)s.pixel] = make_float4(g.nx, g.ny, g.nz, g.hit);
    a.guide[2 * (int64_t)s.pixel + 1] = make_float4(g.px, g.py, g.pz, g.pad);
    a.albedo[s.pixel] = as_float4(albedo);
}

struct FilterArgs : DenoiseFilterLaunch {};

// c_k of a pixel, from global memory: iteration 0 demodulates the frame's image on the way.
template <bool First>
struct GlobalSource {
    const float4* in;
    const float4* guides;
    const float4* albedo;
    int width;
    __device__ Guide guide(int x, int y) const { return load_guide(guides, y * width + x); }
    __device__ Color color(int x, int y, bool hit) const {
        const int q = y * width + x;
        const Color c = as_color(in[q]);
        if (!First || !hit) return c;
        return demodulate(c, as_color(albedo[q]), true);
    }
};

__device__ inline void write_last(const FilterArgs& a, int p, const Color& c, bool hit) {
    const Color r = hit ? remodulate(c, as_color(a.albedo[p]), true) : c;
    if (a.out) a.out[p] = as_float4(r);
    if (a.pixels) a.pixels[p] = pixel_of(r);
}

template <bool First, bool Last>
__global__ __launch_bounds__(kThreads) void filter_kernel(FilterArgs a) {
    const int tileY = (int)blockIdx.x / a.tilesX, tileX = (int)blockIdx.x - tileY * a.tilesX;
    const int x = tileX * kTileW + (int)(threadIdx.x % kTileW), y = tileY * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= a.width || y >= a.height) return;
    const GlobalSource<First> src{a.in, a.guide, a.albedo, a.width};
    const Color c = filter_pixel(src, x, y, a.width, a.height, a.step, a.invPlane, a.invColor2, a.squarings);
    const int p = y * a.width + x;
    if (Last) write_last(a, p, c, is_hit(load_guide(a.guide, p)));
    else a.out[p] = as_float4(c);
}

// c_k of a pixel of the staged tile: plane 0 and 1 hold the guide's halves, plane 2 the colour.
struct TileSource {
    const float4* lds;
    int plane, rowWords, xOrigin, yOrigin, shift;
    __device__ int at(int x, int y) const { return ((y - yOrigin) >> shift) * rowWords + (x - xOrigin); }
    __device__ Guide guide(int x, int y) const {
        const int i = at(x, y);
        return as_guide(lds[i], lds[plane + i]);
    }
    __device__ Color color(int x, int y, bool) const { return as_color(lds[2 * plane + at(x, y)]); }
};

template <bool First, bool Last>
__global__ __launch_bounds__(kThreads) void filter_tiled_kernel(FilterArgs a) {
    extern __shared__ float4 lds[];   // 3 planes of kRowTileStaged * rowWords words
    const int s = a.step, shift = 31 - __clz(s);
    const int rowWords = kRowTileW + 4 * s, plane = kRowTileStaged * rowWords;
    const int tileY = (int)blockIdx.x / a.tilesX, tileX = (int)blockIdx.x - tileY * a.tilesX;
    const int group = tileY / a.residues, residue = tileY - group * a.residues;
    const int x0 = tileX * kRowTileW, y0 = residue + s * kRowTileRows * group;
    const int xOrigin = x0 - 2 * s, yOrigin = y0 - 2 * s;
    for (int i = (int)threadIdx.x; i < plane; i += kThreads) {
        const int row = i / rowWords, col = i - row * rowWords;
        const int x = xOrigin + col, y = yOrigin + row * s;
        float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo, c = lo;   // outside the frame: a miss
        if (x >= 0 && x < a.width && y >= 0 && y < a.height) {
            const int q = y * a.width + x;
            lo = a.guide[2 * (int64_t)q];
            hi = a.guide[2 * (int64_t)q + 1];
            Color v = as_color(a.in[q]);
            if (First && lo.w != 0.0f) v = demodulate(v, as_color(a.albedo[q]), true);
            c = as_float4(v);
        }
        lds[i] = lo;
        lds[plane + i] = hi;
        lds[2 * plane + i] = c;
    }
    __syncthreads();
    const int x = x0 + (int)(threadIdx.x % kRowTileW), y = y0 + (int)(threadIdx.x / kRowTileW) * s;
    if (x >= a.width || y >= a.height) return;
    const TileSource src{lds, plane, rowWords, xOrigin, yOrigin, shift};
    const Color c = filter_pixel(src, x, y, a.width, a.height, s, a.invPlane, a.invColor2, a.squarings);
    const int p = y * a.width + x;
    if (Last) write_last(a, p, c, is_hit(src.guide(x, y)));
    else a.out[p] = as_float4(c);
}

__global__ __launch_bounds__(kThreads) void modulate_kernel(FilterArgs a) {
    const int tileY = (int)blockIdx.x / a.tilesX, tileX = (int)blockIdx.x - tileY * a.tilesX;
    const int x = tileX * kTileW + (int)(threadIdx.x % kTileW), y = tileY * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= a.width || y >= a.height) return;
    const int p = y * a.width + x;
    const bool hit = is_hit(load_guide(a.guide, p));
    const GlobalSource<true> src{a.in, a.guide, a.albedo, a.width};
    write_last(a, p, src.color(x, y, hit), hit);
}

template <class K>
hipError_t launch(K kernel, int grid, hipStream_t s, const FilterArgs& a, int ldsBytes = 0) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)kThreads), (size_t)ldsBytes, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_denoise_features(const DenoiseFeaturesLaunch& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(features_kernel, dim3((unsigned)grid), dim3((unsigned)kThreads), 0, s, FeaturesArgs{a});
    return hipGetLastError();
}

hipError_t launch_denoise_filter(const DenoiseFilterLaunch& a, int grid, hipStream_t s) {
    const FilterArgs f{a};
    if (a.first) return a.last ? launch(filter_kernel<true, true>, grid, s, f) : launch(filter_kernel<true, false>, grid, s, f);
    return a.last ? launch(filter_kernel<false, true>, grid, s, f) : launch(filter_kernel<false, false>, grid, s, f);
}

hipError_t launch_denoise_filter_tiled(const DenoiseFilterLaunch& a, int grid, int ldsBytes, hipStream_t s) {
    const FilterArgs f{a};
    if (a.first)
        return a.last ? launch(filter_tiled_kernel<true, true>, grid, s, f, ldsBytes)
                      : launch(filter_tiled_kernel<true, false>, grid, s, f, ldsBytes);
    return a.last ? launch(filter_tiled_kernel<false, true>, grid, s, f, ldsBytes)
                  : launch(filter_tiled_kernel<false, false>, grid, s, f, ldsBytes);
}

hipError_t launch_denoise_modulate(const DenoiseFilterLaunch& a, int grid, hipStream_t s) {
    return launch(modulate_kernel, grid, s, FilterArgs{a});
}

}  // namespace mrt
