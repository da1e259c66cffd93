// raygen_kernel.hip — the kernels around a frame's traces on the device (gfx950), so a frame
// (primary -> trace -> AO -> trace -> count / reconstruct) never leaves HBM, and their launch
// functions (raygen_kernel.hpp). The C-ABI that calls them is frame_api.cpp.
//
//   primary_kernel                    <- rayGenPrimaryKernel (reference RayGenKernels.cu:79-113)
//   ao_kernel, ao_per_sample_kernel   <- rayGenAOKernel (RayGenKernels.cu:117-227)
//   ao_blocks[_tiled]_kernel          the same rays for a list of blocks of a frame's ray order
//   seed_fill_kernel                  a long frame's batch seeds into device memory
//   count_partial / count_final       <- countHitsKernel (RendererKernels.cu:112-162)
//   reconstruct[_tiled]_kernel        <- reconstructKernel (RendererKernels.cu:60-108)
//
// The per-ray arithmetic is csrc/raygen_common.hpp, the same code the host generator runs.
// These are streaming kernels (32 B written per ray, 16-48 B read) of 256-thread workgroups,
// one thread per output ray or pixel. ao_blocks_tiled_kernel (16 KB) and reconstruct_tiled_kernel
// (17 KB) stage shared values through static LDS; the hit count is a shuffle reduction, one
// partial per block and a one-block final sum (no contended atomics).
//
// Each kernel takes its arguments by value as a file-local struct that adds nothing to the launch
// interface's (PrimaryArgs : PrimaryLaunch, ...): its mangled symbol is then the one it had
// before the interface existed, so profiles and assembly diffs against older builds match by name.
#include "raygen_kernel.hpp"

#include <algorithm>

#include "../../include/mrt.h"   // MRT_RAY_*

namespace mrt {
namespace {

using namespace frame;

struct PrimaryArgs : PrimaryLaunch {};

__global__ __launch_bounds__(kThreads) void primary_kernel(PrimaryArgs a) {
    const int task = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (task >= a.w * a.h) return;
    const int pixel = a.indexToPixel[task];
    a.rays[task] = rg::primary_ray(a.m, rg::make(a.ox, a.oy, a.oz), a.maxDist, a.w, a.h, pixel, a.jx, a.jy);
    if (a.slotToId) a.slotToId[task] = pixel;
    if (a.idToSlot) a.idToSlot[pixel] = task;
}

struct AOArgs : AOLaunch {};

__global__ __launch_bounds__(kThreads) void ao_kernel(AOArgs a) {
    const int task = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (task >= a.numInput) return;
    const int2 res = a.inResults[2 * task];
    const rg::AOBasis b =
        rg::ao_basis(a.inRays[task], res.x, __int_as_float(res.y), a.normals, a.numTris, a.seed, (uint32_t)task);
    const int64_t out = (int64_t)task * a.numSamples;
    for (int i = 0; i < a.numSamples; i++) {
        a.outRays[out + i] = rg::ao_sample(b, i, a.maxDist);
        if (a.outIdToSlot) a.outIdToSlot[out + i] = (int32_t)(out + i);
        if (a.outSlotToId) a.outSlotToId[out + i] = (int32_t)(out + i);
    }
}

// One thread per OUTPUT ray (numSamples > 1): consecutive lanes write consecutive
// 32 B rays (coalesced), each recomputing its input ray's basis (a few dozen
// ALU ops and three L2-resident reads). ao_sample(b, i) depends only on (b, i),
// so the rays are the same bits as ao_kernel's.
__global__ __launch_bounds__(kThreads) void ao_per_sample_kernel(AOArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (int64_t)a.numInput * a.numSamples) return;
    const int task = (int)(gid / a.numSamples), i = (int)(gid - (int64_t)task * a.numSamples);
    const int2 res = a.inResults[2 * task];
    const rg::AOBasis b =
        rg::ao_basis(a.inRays[task], res.x, __int_as_float(res.y), a.normals, a.numTris, a.seed, (uint32_t)task);
    a.outRays[gid] = rg::ao_sample(b, i, a.maxDist);
    if (a.outIdToSlot) a.outIdToSlot[gid] = (int32_t)gid;
    if (a.outSlotToId) a.outSlotToId[gid] = (int32_t)gid;
}

// A frame's secondary rays in block order (mrt_raygen_ao_blocks). The frame's
// RayGen::batching sequence (RayGen.cc:124-142) numbers its rays g = p * S + i
// (input ray p, sample i); batch k holds the inputs [k * P, (k + 1) * P) and hashes
// seed_k + (p - k * P) (RayGen.cc:106, RayGenKernels.cu:122-134). Output ray j is
// ray g = blocks[j / B] * B + j % B of that sequence, so a list of blocks in any
// order comes out as the same bits the batches would hold at those positions —
// a rank's shard generated directly in its trace order, no gather of a frame
// buffer. One thread per output ray: consecutive lanes write consecutive 32-B
// rays; a block id and an input ray are shared by B and S consecutive lanes.
// A frame of at most kMaxBatchSeeds batches carries its seeds in the kernel arguments; a
// longer one reads them from seedTable (device memory, filled on the stream by
// seed_fill_kernel launches that carry kMaxBatchSeeds seeds each in their arguments).
struct AOBlocksArgs : AOBlocksLaunch {};

template <bool kSeedTable>
__device__ inline uint32_t batch_seed(const AOBlocksArgs& a, int batch) {
    return kSeedTable ? a.seedTable[batch] : a.seeds[batch];   // batch < the frame's batches: p < numInput
}

struct SeedFillArgs {
    uint32_t* table;
    int first, count;   // table[first + i] = seeds[i], i < count <= kMaxBatchSeeds
    uint32_t seeds[kMaxBatchSeeds];
};

__global__ __launch_bounds__(kMaxBatchSeeds) void seed_fill_kernel(SeedFillArgs a) {
    const int i = (int)threadIdx.x;
    if (i < a.count) a.table[(int64_t)a.first + i] = a.seeds[i];
}

template <bool kSeedTable>
__global__ __launch_bounds__(kThreads) void ao_blocks_kernel(AOBlocksArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= a.outRays) return;
    const int64_t k = j / a.blockRays;
    const int64_t g = (int64_t)a.blocks[k] * a.blockRays + (j - k * a.blockRays);
    // past the frame's end: the (last-listed) partial block; a block id outside the frame writes nothing
    if (g < 0 || g >= a.totalRays) return;
    const int p = (int)(g / a.numSamples), i = (int)(g - (int64_t)p * a.numSamples);
    const int batch = p / a.batchInputs;
    const int2 res = a.inResults[2 * p];
    const rg::AOBasis b = rg::ao_basis(a.inRays[p], res.x, __int_as_float(res.y), a.normals, a.numTris,
                                       batch_seed<kSeedTable>(a, batch), (uint32_t)(p - batch * a.batchInputs));
    a.out[j] = rg::ao_sample(b, i, a.maxDist);
}

// The same rays when a workgroup's kTileRays outputs lie inside one block (blockRays a
// multiple of kTileRays) and hold whole input rays (numSamples divides kTileRays, at most
// kThreads input rays and at most kThreads samples per ray): each input ray's basis (two trig calls, a normalize, the hash, three
// dependent loads) is computed once by one thread and each sample's hemisphere point once
// per sample index, both through LDS — not once per output ray (S = 8: 8x fewer basis
// evaluations) — then each thread writes kTileRays / kThreads rays (coalesced). Same
// arithmetic, same bits. Four rays per thread: a 2 M-ray shard is 2 025 workgroups, one
// round of the device, so the dependent load chain is paid once, not four times.
template <bool kSeedTable>
__global__ __launch_bounds__(kThreads) void ao_blocks_tiled_kernel(AOBlocksArgs a) {
    __shared__ rg::AOBasis basis[kThreads];
    __shared__ rg::V3 sample[kThreads];
    const int t = (int)threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * kTileRays;
    const int64_t k = j0 / a.blockRays;
    const int64_t g0 = (int64_t)a.blocks[k] * a.blockRays + (j0 - k * a.blockRays);   // a multiple of S
    if (g0 < 0 || g0 >= a.totalRays) return;   // a block id outside the frame (workgroup-uniform): nothing
    const int S = a.numSamples;
    const int perWg = kTileRays / S;
    const int p0 = (int)(g0 / S);
    if (t < perWg && p0 + t < a.numInput) {
        const int p = p0 + t;
        const int batch = p / a.batchInputs;
        const int2 res = a.inResults[2 * p];
        basis[t] = rg::ao_basis(a.inRays[p], res.x, __int_as_float(res.y), a.normals, a.numTris,
                                batch_seed<kSeedTable>(a, batch), (uint32_t)(p - batch * a.batchInputs));
    }
    if (kThreads - 1 - t < S) sample[kThreads - 1 - t] = rg::ao_sample_xyz(kThreads - 1 - t);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kTileRays / kThreads; u++) {
        const int o = u * kThreads + t;
        if (j0 + o >= a.outRays || g0 + o >= a.totalRays) break;
        a.out[j0 + o] = rg::ao_sample_dir(basis[o / S], sample[o % S], a.maxDist);
    }
}

// Per block: hits among its rays (id >= 0, RendererKernels.cu:131), one partial.
__global__ __launch_bounds__(kThreads) void count_partial_kernel(const int4* results, int n, int perBlock,
                                                                int32_t* partial) {
    __shared__ int waveSum[kThreads / 64];
    const int begin = (int)blockIdx.x * perBlock;
    const int end = min(begin + perBlock, n);
    int c = 0;
    for (int i = begin + (int)threadIdx.x; i < end; i += kThreads) c += results[i].x >= 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) waveSum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kThreads / 64; w++) t += waveSum[w];
        partial[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kThreads) void count_final_kernel(const int32_t* partial, int m, int32_t* out) {
    __shared__ int waveSum[kThreads / 64];
    int c = 0;
    for (int i = (int)threadIdx.x; i < m; i += kThreads) c += partial[i];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) waveSum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kThreads / 64; w++) t += waveSum[w];
        *out = t;
    }
}

struct ReconstructArgs : ReconstructLaunch {};

// fromABGR / toABGR of RendererKernels.cu:38-56 (device variant: truncating, not rounding).
__device__ inline float4 from_abgr(uint32_t c) {
    const float k = 1.0f / 255.0f;
    return make_float4((float)(c & 0xFF) * k, (float)((c >> 8) & 0xFF) * k, (float)((c >> 16) & 0xFF) * k,
                       (float)(c >> 24) * k);
}
__device__ inline uint32_t to_abgr(float4 v) {
    return (uint32_t)(fminf(fmaxf(v.x, 0.0f), 1.0f) * 255.0f) |
           ((uint32_t)(fminf(fmaxf(v.y, 0.0f), 1.0f) * 255.0f) << 8) |
           ((uint32_t)(fminf(fmaxf(v.z, 0.0f), 1.0f) * 255.0f) << 16) |
           ((uint32_t)(fminf(fmaxf(v.w, 0.0f), 1.0f) * 255.0f) << 24);
}

__device__ inline void add_sample(float4& c, int tri, bool isPrimary, bool isAO, const uint32_t* shaded) {
    float4 add;
    if (tri == -1) add = isPrimary ? make_float4(0.2f, 0.4f, 0.8f, 1.0f) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    else add = isAO ? make_float4(0.0f, 0.0f, 0.0f, 1.0f) : from_abgr(shaded[tri]);
    c.x += add.x; c.y += add.y; c.z += add.z; c.w += add.w;
}

// Average -> AO background -> diffuse modulation -> one ABGR pixel (RendererKernels.cu:96-107).
__device__ inline void finish_pixel(const ReconstructArgs& a, float4 c, int primarySlot) {
    const float4 bg = make_float4(0.2f, 0.4f, 0.8f, 1.0f);
    const float inv = 1.0f / (float)a.numRaysPerPrimary;
    c.x *= inv; c.y *= inv; c.z *= inv; c.w *= inv;
    const int tri = a.primaryResults[primarySlot].x;
    if (a.rayType == MRT_RAY_AO && tri == -1) c = bg;
    if (a.rayType == MRT_RAY_DIFFUSE) {
        const float4 m = tri == -1 ? bg : from_abgr(a.triMaterialColor[tri]);
        c.x *= m.x; c.y *= m.y; c.z *= m.z; c.w *= m.w;
    }
    a.pixels[a.primarySlotToId[primarySlot]] = to_abgr(c);
}

// One thread per primary ray of the batch: average the batch rays' colours
// (background / white / shaded triangle colour), modulate by the primary hit's
// material for diffuse, write one ABGR pixel (RendererKernels.cu:60-108).
// General form: any batchIdToSlot (gathers), and the primary batch.
__global__ __launch_bounds__(kThreads) void reconstruct_kernel(ReconstructArgs a) {
    const int task = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (task >= a.numPrimary) return;
    const int n = a.numRaysPerPrimary;
    const bool isPrimary = a.rayType == MRT_RAY_PRIMARY, isAO = a.rayType == MRT_RAY_AO;
    const int primarySlot = a.firstPrimary + task;
    const int batchBase = isPrimary ? a.primarySlotToId[primarySlot] : task * n;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = 0; i < n; i++) {
        const int slot = a.batchIdToSlot ? a.batchIdToSlot[batchBase + i] : (isPrimary ? primarySlot : batchBase + i);
        add_sample(c, a.batchResults[slot].x, isPrimary, isAO, a.triShadedColor);
    }
    finish_pixel(a, c, primarySlot);
}

// Identity-layout AO/diffuse batches (mrt_raygen_ao's): the block's n rays per
// primary are one contiguous run of results, so the hit ids are staged through
// LDS with coalesced loads (consecutive lanes, consecutive results) in tiles of
// kTileSamples per primary, then each thread sums its own samples in ray order
// (bit-identical to reconstruct_kernel). Row stride kTileSamples + 1 keeps the
// per-thread LDS reads conflict-free.
constexpr int kTileSamples = 16;
__global__ __launch_bounds__(kThreads) void reconstruct_tiled_kernel(ReconstructArgs a) {
    __shared__ int ids[kThreads * (kTileSamples + 1)];
    const int n = a.numRaysPerPrimary;
    const bool isAO = a.rayType == MRT_RAY_AO;
    const int taskBase = (int)blockIdx.x * kThreads;
    const int nTasks = min(kThreads, a.numPrimary - taskBase);
    const int t = (int)threadIdx.x;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int s0 = 0; s0 < n; s0 += kTileSamples) {
        const int ns = min(kTileSamples, n - s0);
        const int cnt = nTasks * ns;
        __syncthreads();
        for (int e = t; e < cnt; e += kThreads) {
            const int tt = e / ns, ss = e - tt * ns;
            ids[tt * (kTileSamples + 1) + ss] = a.batchResults[(int64_t)(taskBase + tt) * n + s0 + ss].x;
        }
        __syncthreads();
        if (t < nTasks)
            for (int ss = 0; ss < ns; ss++) add_sample(c, ids[t * (kTileSamples + 1) + ss], false, isAO, a.triShadedColor);
    }
    if (t < nTasks) finish_pixel(a, c, a.firstPrimary + taskBase + t);
}

template <class K, class A>
hipError_t launch(K kernel, int grid, int threads, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_primary(const PrimaryLaunch& a, int grid, hipStream_t s) {
    return launch(primary_kernel, grid, kThreads, s, PrimaryArgs{a});
}

hipError_t launch_ao(const AOLaunch& a, int grid, hipStream_t s) {
    return launch(a.numSamples > 1 ? ao_per_sample_kernel : ao_kernel, grid, kThreads, s, AOArgs{a});
}

hipError_t launch_seed_table(uint32_t* table, const uint32_t* seeds, int64_t count, hipStream_t s) {
    SeedFillArgs f{};
    f.table = table;
    for (int64_t first = 0; first < count; first += kMaxBatchSeeds) {
        f.first = (int)first;
        f.count = (int)std::min<int64_t>(kMaxBatchSeeds, count - first);
        for (int k = 0; k < f.count; k++) f.seeds[k] = seeds[first + k];
        if (hipError_t e = launch(seed_fill_kernel, 1, kMaxBatchSeeds, s, f)) return e;
    }
    return hipSuccess;
}

hipError_t launch_ao_blocks(const AOBlocksLaunch& a, bool tiled, int grid, hipStream_t s) {
    if (a.seedTable) return launch(tiled ? ao_blocks_tiled_kernel<true> : ao_blocks_kernel<true>, grid, kThreads, s, AOBlocksArgs{a});
    return launch(tiled ? ao_blocks_tiled_kernel<false> : ao_blocks_kernel<false>, grid, kThreads, s, AOBlocksArgs{a});
}

hipError_t launch_count_hits(const int4* results, int n, int perBlock, int blocks, int32_t* partial, int32_t* hitCount,
                             hipStream_t s) {
    if (blocks > 0)
        hipLaunchKernelGGL(count_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, results, n, perBlock, partial);
    hipLaunchKernelGGL(count_final_kernel, dim3(1), dim3(kThreads), 0, s, partial, blocks, hitCount);
    return hipGetLastError();
}

hipError_t launch_reconstruct(const ReconstructLaunch& a, int grid, hipStream_t s) {
    const bool tiled = a.rayType != MRT_RAY_PRIMARY && !a.batchIdToSlot;
    return launch(tiled ? reconstruct_tiled_kernel : reconstruct_kernel, grid, kThreads, s, ReconstructArgs{a});
}

}  // namespace mrt
