// shard_kernel.hpp — launch interface between the C-ABI glue (frame_api.cpp: mrt_shard_blocks)
// and the gfx950 kernels that list a rank's blocks of a frame's secondary rays and put them in
// live-first trace order (shard_kernel.hip). Grids, tiles and scratch sizes come from the plan
// (frame_plan.hpp: OrderPlan); one function is one of its paths.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mrt {

// A rank's block list: entry j is block rank + j * world of the frame.
struct ShardLaunch {
    const int2* results;     // primary RayResult viewed as int2 pairs
    int numPrimary, numSamples, blockRays, world, rank, numBlocks;   // numBlocks: listed (this rank's)
    int64_t totalRays;
    int32_t* out;            // the block list; first the keys (block_live_kernel), then the ordered ids
};

// The list in frame order.
hipError_t launch_shard_list(const ShardLaunch& a, int grid, hipStream_t s);
// The list in live-first order, at most frame::kOrderMax entries: the keys, then their sort
// and the ids by one workgroup. No scratch.
hipError_t launch_shard_order(const ShardLaunch& a, int liveGrid, hipStream_t s);
// A longer list, in numTiles tiles of kOrderMax entries: the keys, the tiles' sorts, the scan of
// their key counts, the scatter. table: (kKeyMax + 1) * numTiles ints, 16-byte aligned;
// pairs: numBlocks words.
hipError_t launch_shard_order_tiled(const ShardLaunch& a, int liveGrid, int numTiles, int32_t* table, uint32_t* pairs,
                                    hipStream_t s);

}  // namespace mrt
