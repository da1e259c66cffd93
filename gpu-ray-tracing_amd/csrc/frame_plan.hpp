// frame_plan.hpp — the integer planning of the frame path's exports (frame_api.cpp): a rank's
// share of a frame's blocks, the path its block list takes to its order and the scratch that
// needs, the consistency checks and the grid of the block ray generator, the hit count's
// partials, and the 1-D grids of the rest.
// Plain C++ with no HIP in it (like launch_plan.hpp): frame_api.cpp feeds it the caller's counts,
// tests/cpp/frame_plan_driver.cpp runs it on the CPU.
//
// Every size and grid is computed in int64_t and narrowed once, where its range is known: the
// exports' counts are int32, a frame holds at most INT32_MAX rays (checked here, first), and what
// follows from those fits an int.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/mrt.h"
#include "frame_limits.hpp"

namespace mrt {

// Workgroups of `threads` threads that give each of n >= 0 items one thread; -1 (which no launch
// accepts) when that is no int. No count an export lets through gets there.
int grid_1d(int64_t n, int threads = frame::kThreads);

// Rank `rank`'s share of a frame of numPrimary * numSamples rays in blocks of blockRays, block i
// to rank i % world. All arguments valid (counts >= 0, sizes >= 1, rank < world).
struct ShardExtent {
    int rc = MRT_OK;        // MRT_ERR_TOO_LARGE: more than INT32_MAX frame rays (nothing else set)
    int64_t total = 0;      // the frame's rays
    int64_t nb = 0;         // its blocks; the last one may be partial
    int mine = 0;           // this rank's blocks
    bool lastMine = false;  // the frame's last block is among them
    int64_t numRays = 0;    // the rays of this rank's blocks
};
ShardExtent shard_extent(int numPrimary, int numSamples, int blockRays, int world, int rank);

// How a list of `mine` blocks gets its order (order 0: frame order, 1: live-first).
enum class OrderPath : int {
    none = 0,           // no blocks: nothing to launch
    list = 1,           // frame order: one launch
    oneWorkgroup = 2,   // at most kOrderMax entries: the keys, one workgroup's sort
    tiled = 3,          // more: tiles of kOrderMax entries, with scratch
};
struct OrderPlan {
    OrderPath path = OrderPath::none;
    int grid = 0;              // list: the list launch's; oneWorkgroup / tiled: block_live_kernel's (a wave per entry)
    int numTiles = 0;          // tiled only, as are the sizes below
    int64_t tableWords = 0;    // the key-by-tile table, (kKeyMax + 1) * numTiles, first in the scratch
    int64_t scratchWords = 0;  // the table and one word per entry (the tile-sorted pairs)
    size_t scratchBytes = 0;
};
OrderPlan plan_order(int mine, int order);

// mrt_raygen_ao_blocks' counts: the checks in the export's order, then the launch.
struct AOBlocksPlan {
    int rc = MRT_OK;            // with `why`, the refusal; the fields below are set up to the failing check
    const char* why = "";
    int64_t total = 0;          // numInputRays * numSamples
    int64_t needBatches = 0;    // batches the frame's input rays span
    bool empty = false;         // numOutRays == 0: accepted, nothing to launch
    bool tiled = false;         // ao_blocks_tiled_kernel applies
    int grid = 0;
    bool seedsInArgs = false;   // needBatches <= kMaxBatchSeeds: no seed table
};
AOBlocksPlan plan_ao_blocks(int numInputRays, int numSamples, int numBatches, int batchInputRays, int numBlocks,
                            int blockRays, int64_t numOutRays);

// mrt_count_hits: `blocks` (<= kCountBlocks) partials of perBlock (a positive multiple of
// kThreads) results each cover numRays >= 0, none of them empty; no rays, no blocks.
struct CountPlan {
    int perBlock = 0, blocks = 0;
};
CountPlan plan_count(int numRays);

}  // namespace mrt
