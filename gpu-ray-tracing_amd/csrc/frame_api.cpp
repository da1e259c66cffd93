// frame_api.cpp — the C-ABI of a frame's steps around its traces: mrt_raygen_primary /
// _primary_subpixel / _ao / _ao_blocks, mrt_shard_blocks, mrt_count_hits and mrt_reconstruct.
// Per export: the argument checks, the plan (frame_plan.cpp: counts, grids, scratch sizes), the
// launches (raygen_kernel.hip, shard_kernel.hip). Everything is enqueued on the caller's
// stream; nothing waits on the host and no state outlives a call.
//
//   mrt_raygen_primary  <- RayGen::primary (reference RayGen.cc:50-72)
//   mrt_raygen_ao       <- RayGen::ao (RayGen.cc:77-120)
//   mrt_count_hits      <- launch_countHitsKernel (RendererKernels.cu:189-)
//   mrt_reconstruct     <- launch_reconstructKernel (Renderer.cc:421-445)
#include <string>

#include "api_common.hpp"
#include "frame_plan.hpp"
#include "raygen_kernel.hpp"
#include "shard_kernel.hpp"

using mrt::fail;
using mrt::hipFail;
using mrt::launched;

namespace {

// Whether [p, p + bytes) lies in memory the device can address, as far as the runtime can tell
// without touching the stream: p is registered with it (device, managed or pinned host memory)
// and, where it reports the allocation's range, the range holds the bytes. False for any other
// pointer, and when there is no device.
bool device_memory_holds(const void* p, size_t bytes) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();   // a query's failure is an answer, not a launch error
        return false;
    }
    if (at.type == hipMemoryTypeUnregistered) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return true;               // registered, but of a kind the runtime gives no range for
    }
    return static_cast<const char*>(p) + bytes <= static_cast<const char*>(base) + size;
}

}  // namespace

extern "C" {

int mrt_raygen_primary(const float nscreenToWorld[16], const float origin[3], float maxDist, int32_t w, int32_t h,
                       const int32_t* indexToPixel, void* rays, int32_t* slotToId, int32_t* idToSlot, void* stream) {
    return mrt_raygen_primary_subpixel(nscreenToWorld, origin, maxDist, w, h, 0.5f, 0.5f, indexToPixel, rays, slotToId,
                                       idToSlot, stream);
}

int mrt_raygen_primary_subpixel(const float nscreenToWorld[16], const float origin[3], float maxDist, int32_t w,
                                int32_t h, float jx, float jy, const int32_t* indexToPixel, void* rays,
                                int32_t* slotToId, int32_t* idToSlot, void* stream) {
    if (!nscreenToWorld || !origin || !indexToPixel || !rays) return fail(MRT_ERR_INVALID_ARG, "null argument");
    if (w <= 0 || h <= 0 || (int64_t)w * h > INT32_MAX) return fail(MRT_ERR_INVALID_ARG, "bad image size");
    if (!(jx >= 0.0f && jx < 1.0f && jy >= 0.0f && jy < 1.0f)) return fail(MRT_ERR_INVALID_ARG, "subpixel offset outside [0, 1)");
    mrt::PrimaryLaunch a{};
    a.jx = jx;
    a.jy = jy;
    for (int i = 0; i < 16; i++) a.m[i] = nscreenToWorld[i];
    a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
    a.maxDist = maxDist;
    a.w = w; a.h = h;
    a.indexToPixel = indexToPixel;
    a.rays = static_cast<mrt::rg::RayRec*>(rays);
    a.slotToId = slotToId;
    a.idToSlot = idToSlot;
    return launched(mrt::launch_primary(a, mrt::grid_1d((int64_t)w * h), static_cast<hipStream_t>(stream)),
                    "raygen primary launch");
}

int mrt_raygen_ao(const void* inRays, const void* inResults, int32_t numInputRays, const float* triNormals,
                  int64_t numTris, int32_t numSamples, float maxDist, uint32_t seed, void* outRays,
                  int32_t* outIdToSlot, int32_t* outSlotToId, void* stream) {
    if (numInputRays < 0 || numSamples < 1) return fail(MRT_ERR_INVALID_ARG, "bad ray/sample count");
    if (numInputRays == 0) return MRT_OK;
    if (!inRays || !inResults || !outRays || (numTris > 0 && !triNormals))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    const int64_t total = (int64_t)numInputRays * numSamples;
    if (total > INT32_MAX) return fail(MRT_ERR_TOO_LARGE, "too many output rays");
    mrt::AOLaunch a{};
    a.inRays = static_cast<const mrt::rg::RayRec*>(inRays);
    a.inResults = static_cast<const int2*>(inResults);
    a.numInput = numInputRays;
    a.normals = triNormals;
    a.numTris = numTris;
    a.numSamples = numSamples;
    a.maxDist = maxDist;
    a.seed = seed;
    a.outRays = static_cast<mrt::rg::RayRec*>(outRays);
    a.outIdToSlot = outIdToSlot;
    a.outSlotToId = outSlotToId;
    // one thread per output ray (numSamples 1: per input ray, the same count)
    return launched(mrt::launch_ao(a, mrt::grid_1d(total), static_cast<hipStream_t>(stream)), "raygen ao launch");
}

int mrt_raygen_ao_blocks(const void* inRays, const void* inResults, int32_t numInputRays, const float* triNormals,
                         int64_t numTris, int32_t numSamples, float maxDist, const uint32_t* batchSeeds,
                         int32_t numBatches, int32_t batchInputRays, const int32_t* blocks, int32_t numBlocks,
                         int32_t blockRays, int64_t numOutRays, void* outRays, void* stream) {
    const mrt::AOBlocksPlan p =
        mrt::plan_ao_blocks(numInputRays, numSamples, numBatches, batchInputRays, numBlocks, blockRays, numOutRays);
    if (p.rc != MRT_OK) return fail(p.rc, p.why);
    if (p.empty) return MRT_OK;
    if (!inRays || !inResults || !outRays || !blocks || !batchSeeds || (numTris > 0 && !triNormals))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    mrt::AOBlocksLaunch a{};
    a.inRays = static_cast<const mrt::rg::RayRec*>(inRays);
    a.inResults = static_cast<const int2*>(inResults);
    a.numInput = numInputRays;
    a.normals = triNormals;
    a.numTris = numTris;
    a.numSamples = numSamples;
    a.maxDist = maxDist;
    a.batchInputs = batchInputRays;
    a.blockRays = blockRays;
    a.totalRays = p.total;
    a.outRays = numOutRays;
    a.blocks = blocks;
    a.out = static_cast<mrt::rg::RayRec*>(outRays);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.seedsInArgs) {
        for (int64_t k = 0; k < p.needBatches; k++) a.seeds[k] = batchSeeds[k];
        return launched(mrt::launch_ao_blocks(a, p.tiled, p.grid, s), "raygen ao blocks launch");
    }
    // More batches than the arguments hold: the seeds go to stream-ordered scratch through fill
    // launches whose arguments carry them (no copy from pageable memory, no host sync), the
    // generator reads them there.
    mrt::StreamScratch table;
    if (hipError_t e = table.alloc((size_t)p.needBatches * sizeof(uint32_t), s)) return hipFail(e, "hipMallocAsync(batch seeds)");
    a.seedTable = table.as<uint32_t>();
    hipError_t e = mrt::launch_seed_table(table.as<uint32_t>(), batchSeeds, p.needBatches, s);
    if (e == hipSuccess) e = mrt::launch_ao_blocks(a, p.tiled, p.grid, s);
    return launched(e, "raygen ao blocks launch", table, "hipFreeAsync(batch seeds)");
}

int mrt_shard_blocks(const void* primaryResults, int32_t numPrimary, int32_t numSamples, int32_t blockRays,
                     int32_t world, int32_t rank, int32_t order, int32_t* blocks, int32_t capacity, int32_t* numBlocks,
                     int64_t* numRays, void* stream) {
    if (numPrimary < 0 || numSamples < 1 || blockRays < 1 || world < 1 || rank < 0 || rank >= world ||
        (order != 0 && order != 1) || !numBlocks || !numRays)
        return fail(MRT_ERR_INVALID_ARG, "bad shard arguments");
    const mrt::ShardExtent x = mrt::shard_extent(numPrimary, numSamples, blockRays, world, rank);
    if (x.rc != MRT_OK) return fail(x.rc, "too many frame rays");
    *numBlocks = x.mine;
    *numRays = x.numRays;
    if (x.mine == 0 || !blocks) return MRT_OK;   // blocks NULL: a size query
    if (capacity < x.mine) return fail(MRT_ERR_TOO_LARGE, "block list capacity below the shard's blocks");
    if (order == 1 && !primaryResults) return fail(MRT_ERR_INVALID_ARG, "null primary results");
    hipStream_t s = static_cast<hipStream_t>(stream);
    mrt::ShardLaunch a{};
    a.results = static_cast<const int2*>(primaryResults);
    a.numPrimary = numPrimary;
    a.numSamples = numSamples;
    a.blockRays = blockRays;
    a.world = world;
    a.rank = rank;
    a.numBlocks = x.mine;
    a.totalRays = x.total;
    a.out = blocks;
    const mrt::OrderPlan p = mrt::plan_order(x.mine, order);
    if (p.path == mrt::OrderPath::list) return launched(mrt::launch_shard_list(a, p.grid, s), "shard block list launch");
    if (p.path == mrt::OrderPath::oneWorkgroup) return launched(mrt::launch_shard_order(a, p.grid, s), "shard order launch");
    // A long list is written by many workgroups over four launches: before anything is taken or
    // launched, the list the caller gave must really be there — capacity is the caller's word, the
    // allocation's extent the runtime's — and so must the results it is ordered by.
    if (!device_memory_holds(blocks, (size_t)x.mine * sizeof(int32_t)))
        return fail(MRT_ERR_TOO_LARGE, "no device memory of the shard's blocks behind the block list (" +
                                           std::to_string(x.mine) + " entries)");
    if (!device_memory_holds(primaryResults, (size_t)numPrimary * 4 * sizeof(int32_t)))
        return fail(MRT_ERR_INVALID_ARG, "no device memory of numPrimary results behind primaryResults");
    // The key-by-tile table first (its int4 accesses stay aligned), then the tile-sorted pairs.
    mrt::StreamScratch scratch;
    if (hipError_t e = scratch.alloc(p.scratchBytes, s)) return hipFail(e, "hipMallocAsync(shard order scratch)");
    int32_t* table = scratch.as<int32_t>();
    return launched(mrt::launch_shard_order_tiled(a, p.grid, p.numTiles, table,
                                                  reinterpret_cast<uint32_t*>(table + p.tableWords), s),
                    "shard order launch", scratch, "hipFreeAsync(shard order scratch)");
}

int mrt_count_hits(const void* results, int32_t numRays, int32_t* hitCount, void* stream) {
    if (!hitCount || numRays < 0 || (numRays > 0 && !results)) return fail(MRT_ERR_INVALID_ARG, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const mrt::CountPlan p = mrt::plan_count(numRays);
    mrt::StreamScratch partial;   // one per block (and one more, so there is always an allocation)
    if (hipError_t e = partial.alloc((size_t)(p.blocks + 1) * sizeof(int32_t), s)) return hipFail(e, "hipMallocAsync(count partials)");
    return launched(mrt::launch_count_hits(static_cast<const int4*>(results), numRays, p.perBlock, p.blocks,
                                           partial.as<int32_t>(), hitCount, s),
                    "count hits launch", partial, "hipFreeAsync(count partials)");
}

int mrt_reconstruct(int32_t rayType, int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                    const int32_t* primarySlotToId, const void* primaryResults, const int32_t* batchIdToSlot,
                    const void* batchResults, const uint32_t* triMaterialColor, const uint32_t* triShadedColor,
                    uint32_t* pixels, void* stream) {
    if (rayType < MRT_RAY_PRIMARY || rayType > MRT_RAY_DIFFUSE) return fail(MRT_ERR_INVALID_ARG, "bad ray type");
    if (numRaysPerPrimary < 1 || firstPrimary < 0 || numPrimary < 0 ||
        (rayType == MRT_RAY_PRIMARY && numRaysPerPrimary != 1))
        return fail(MRT_ERR_INVALID_ARG, "bad batch shape");
    if ((int64_t)numPrimary * numRaysPerPrimary > INT32_MAX || (int64_t)firstPrimary + numPrimary > INT32_MAX)
        return fail(MRT_ERR_TOO_LARGE, "too many rays");
    if (numPrimary == 0) return MRT_OK;
    if (!primarySlotToId || !primaryResults || !batchResults || !pixels ||
        (rayType != MRT_RAY_AO && !triShadedColor) || (rayType == MRT_RAY_DIFFUSE && !triMaterialColor))
        return fail(MRT_ERR_INVALID_ARG, "null argument");
    mrt::ReconstructLaunch a{};
    a.numRaysPerPrimary = numRaysPerPrimary;
    a.firstPrimary = firstPrimary;
    a.numPrimary = numPrimary;
    a.rayType = rayType;
    a.primarySlotToId = primarySlotToId;
    a.primaryResults = static_cast<const int4*>(primaryResults);
    a.batchIdToSlot = batchIdToSlot;
    a.batchResults = static_cast<const int4*>(batchResults);
    a.triMaterialColor = triMaterialColor;
    a.triShadedColor = triShadedColor;
    a.pixels = pixels;
    return launched(mrt::launch_reconstruct(a, mrt::grid_1d(numPrimary), static_cast<hipStream_t>(stream)),
                    "reconstruct launch");
}

}  // extern "C"
