// svgf_kernel.hip — the variance-guided filter's kernels on the device (gfx950) (svgf_kernel.hpp).
// The C-ABI that calls them is svgf_api.cpp.
//
//   accumulate_kernel   temporal_kernel.hip's accumulate_kernel with the moments: one lane per pixel,
//                       the same loads plus up to four taps of the previous moments (16 bytes each)
//                       at the addresses the history's taps have, and one more 16-byte store. The
//                       reprojection is written twice in svgf_common.hpp and once in the code: both
//                       calls inline and their common loads and tests merge. <Tiled> as there
//   variance_kernel     c_0, one lane per pixel of a 32 x 8 tile. A pixel whose history holds four
//                       frames or more reads its own image, guide, albedo and moments and is done;
//                       the 7 x 7 window of a shorter history sits behind a branch that is uniform
//                       over most waves from the fourth frame on, and its 49 taps (a guide and a
//                       moments record each) come through the caches: no LDS staging was tried
//   iterate_kernel      one iteration, one lane per pixel of a 32 x 8 tile, every tap loaded through
//                       the caches, as denoise_kernel.hip's filter_kernel
//   iterate_tiled_kernel   the same iteration with the 5 x 5 taps staged in LDS, in the geometry of
//                       denoise_kernel.hip's filter_tiled_kernel: 64 consecutive columns of 4 rows
//                       `step` apart, 8 staged rows of 64 + 4 * step columns, three planes of 16-byte
//                       words (guide low, guide high, colour with the variance in w). The nine
//                       adjacent variances of the 3 x 3 Gaussian are not in a tile staged a step
//                       apart: at every step they are read from global memory (a hit flag and a
//                       variance, 4 bytes each), through the caches, rather than widening the tile
//   <Last> remodulates and writes imageOut, the pixels and varianceOut
//
// No workgroup waits on another and there are no atomics: a launch reads one image and writes
// another, and the iteration boundary is the launch boundary. The per-pixel arithmetic is
// csrc/svgf_common.hpp, the same code the host runs (csrc/host/svgf.cpp); this file is built without
// denormal flushing (Makefile), so the bits are the host's.
#include "svgf_kernel.hpp"

#include "record_device.hpp"
#include "svgf_limits.hpp"
#include "temporal_limits.hpp"

namespace mrt {
namespace {

using denoise::Color;
using denoise::Guide;

struct AccumulateArgs : SvgfAccumulateLaunch {};

struct AccumulateSource {
    const AccumulateArgs& a;
    __device__ Color image(int p) const { return as_color(a.image[p]); }
    __device__ Guide guide(int p) const { return load_guide(a.guide, p); }
    __device__ Color albedo(int p) const { return as_color(a.albedo[p]); }
    __device__ Color prev_position(int p) const { return as_color(a.prevPosition[p]); }
    __device__ Guide prev_guide(int q) const { return load_guide(a.prevGuide, q); }
    __device__ Color prev_history(int q) const { return as_color(a.prevHistory[q]); }
    __device__ Color prev_moments(int q) const { return as_color(a.prevMoments[q]); }
};

template <bool Tiled>
__global__ __launch_bounds__(temporal::kThreads) void accumulate_kernel(AccumulateArgs a) {
    int p;
    if (Tiled) {
        const int tileY = (int)blockIdx.x / a.tilesX, tileX = (int)blockIdx.x - tileY * a.tilesX;
        const int x = tileX * temporal::kTileW + (int)(threadIdx.x % temporal::kTileW);
        const int y = tileY * temporal::kTileH + (int)(threadIdx.x / temporal::kTileW);
        if (x >= a.k.width || y >= a.k.height) return;
        p = y * a.k.width + x;
    } else {
        p = (int)(blockIdx.x * temporal::kThreads + threadIdx.x);   // < 2^26 + 256
        if (p >= a.k.width * a.k.height) return;
    }
    Color history, moments, result;
    svgf::accumulate_pixel(AccumulateSource{a}, a.k, p, history, moments, result);
    a.history[p] = as_float4(history);
    a.moments[p] = as_float4(moments);
    if (a.imageOut) a.imageOut[p] = as_float4(result);
    if (a.pixels) a.pixels[p] = denoise::pixel_of(result);
}

using namespace svgf;

struct FilterArgs : SvgfFilterLaunch {};

__device__ inline bool tile_pixel(const FilterArgs& a, int& x, int& y) {
    const int tileY = (int)blockIdx.x / a.tilesX, tileX = (int)blockIdx.x - tileY * a.tilesX;
    x = tileX * kTileW + (int)(threadIdx.x % kTileW);
    y = tileY * kTileH + (int)(threadIdx.x / kTileW);
    return x < a.width && y < a.height;
}

__device__ inline void write_last(const FilterArgs& a, int p, const Color& c, bool hit) {
    const Color v{c.r, c.g, c.b, a.image[p].w};
    const Color r = hit ? denoise::remodulate(v, as_color(a.albedo[p]), true) : v;
    if (a.out) a.out[p] = as_float4(r);
    if (a.pixels) a.pixels[p] = denoise::pixel_of(r);
    if (a.varianceOut) a.varianceOut[p] = c.a;
}

struct VarianceSource {
    const FilterArgs& a;
    __device__ Guide guide(int x, int y) const { return load_guide(a.guide, y * a.width + x); }
    __device__ Color image(int x, int y) const { return as_color(a.image[y * a.width + x]); }
    __device__ Color albedo(int x, int y) const { return as_color(a.albedo[y * a.width + x]); }
    __device__ Color moments(int x, int y) const { return as_color(a.moments[y * a.width + x]); }
};

template <bool Last>
__global__ __launch_bounds__(kThreads) void variance_kernel(FilterArgs a) {
    int x, y;
    if (!tile_pixel(a, x, y)) return;
    const Color c = variance_pixel(VarianceSource{a}, x, y, a.width, a.height, a.invPlane, a.squarings);
    const int p = y * a.width + x;
    if (Last) write_last(a, p, c, denoise::is_hit(load_guide(a.guide, p)));
    else a.out[p] = as_float4(c);
}

// An adjacent pixel's hit flag and variance, from global memory in both iteration kernels.
struct NearGlobal {
    const float4* in;
    const float4* guides;
    int width;
    __device__ bool near_hit(int x, int y) const {
        return reinterpret_cast<const float*>(guides)[8 * (int64_t)(y * width + x) + 3] != 0.0f;
    }
    __device__ float near_variance(int x, int y) const {
        return reinterpret_cast<const float*>(in)[4 * (int64_t)(y * width + x) + 3];
    }
};

struct GlobalSource : NearGlobal {
    __device__ Guide guide(int x, int y) const { return load_guide(guides, y * width + x); }
    __device__ Color color(int x, int y) const { return as_color(in[y * width + x]); }
};

template <bool Last>
__global__ __launch_bounds__(kThreads) void iterate_kernel(FilterArgs a) {
    int x, y;
    if (!tile_pixel(a, x, y)) return;
    const GlobalSource src{{a.in, a.guide, a.width}};
    const Color c = filter_pixel(src, x, y, a.width, a.height, a.step, a.invPlane, a.sigmaLum2, a.squarings);
    const int p = y * a.width + x;
    if (Last) write_last(a, p, c, denoise::is_hit(load_guide(a.guide, p)));
    else a.out[p] = as_float4(c);
}

// c_k of a pixel of the staged tile: plane 0 and 1 hold the guide's halves, plane 2 the colour.
struct TileSource : NearGlobal {
    const float4* lds;
    int plane, rowWords, xOrigin, yOrigin, shift;
    __device__ int at(int x, int y) const { return ((y - yOrigin) >> shift) * rowWords + (x - xOrigin); }
    __device__ Guide guide(int x, int y) const {
        const int i = at(x, y);
        return as_guide(lds[i], lds[plane + i]);
    }
    __device__ Color color(int x, int y) const { return as_color(lds[2 * plane + at(x, y)]); }
};

template <bool Last>
__global__ __launch_bounds__(kThreads) void iterate_tiled_kernel(FilterArgs a) {
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
            c = a.in[q];
        }
        lds[i] = lo;
        lds[plane + i] = hi;
        lds[2 * plane + i] = c;
    }
    __syncthreads();
    const int x = x0 + (int)(threadIdx.x % kRowTileW), y = y0 + (int)(threadIdx.x / kRowTileW) * s;
    if (x >= a.width || y >= a.height) return;
    const TileSource src{{a.in, a.guide, a.width}, lds, plane, rowWords, xOrigin, yOrigin, shift};
    const Color c = filter_pixel(src, x, y, a.width, a.height, s, a.invPlane, a.sigmaLum2, a.squarings);
    const int p = y * a.width + x;
    if (Last) write_last(a, p, c, denoise::is_hit(src.guide(x, y)));
    else a.out[p] = as_float4(c);
}

template <class K>
hipError_t launch(K kernel, int grid, hipStream_t s, const FilterArgs& a, int ldsBytes = 0) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)kThreads), (size_t)ldsBytes, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_svgf_accumulate(const SvgfAccumulateLaunch& a, int grid, bool tiled, hipStream_t s) {
    const dim3 g((unsigned)grid), b((unsigned)temporal::kThreads);
    if (tiled) hipLaunchKernelGGL(accumulate_kernel<true>, g, b, 0, s, AccumulateArgs{a});
    else hipLaunchKernelGGL(accumulate_kernel<false>, g, b, 0, s, AccumulateArgs{a});
    return hipGetLastError();
}

hipError_t launch_svgf_variance(const SvgfFilterLaunch& a, int grid, hipStream_t s) {
    const FilterArgs f{a};
    return a.last ? launch(variance_kernel<true>, grid, s, f) : launch(variance_kernel<false>, grid, s, f);
}

hipError_t launch_svgf_iterate(const SvgfFilterLaunch& a, int grid, hipStream_t s) {
    const FilterArgs f{a};
    return a.last ? launch(iterate_kernel<true>, grid, s, f) : launch(iterate_kernel<false>, grid, s, f);
}

hipError_t launch_svgf_iterate_tiled(const SvgfFilterLaunch& a, int grid, int ldsBytes, hipStream_t s) {
    const FilterArgs f{a};
    return a.last ? launch(iterate_tiled_kernel<true>, grid, s, f, ldsBytes) : launch(iterate_tiled_kernel<false>, grid, s, f, ldsBytes);
}

}  // namespace mrt
