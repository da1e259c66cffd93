// frame_plan.cpp — the frame path's integer planning (frame_plan.hpp). Host compiler, no HIP.
#include "frame_plan.hpp"

namespace mrt {

using namespace frame;

namespace {
constexpr int64_t ceil_div(int64_t n, int64_t d) { return (n + d - 1) / d; }
}  // namespace

int grid_1d(int64_t n, int threads) {
    const int64_t g = n >= 0 && threads > 0 ? ceil_div(n, threads) : -1;
    return g <= INT32_MAX ? (int)g : -1;
}

ShardExtent shard_extent(int numPrimary, int numSamples, int blockRays, int world, int rank) {
    ShardExtent x;
    const int64_t total = (int64_t)numPrimary * numSamples;
    if (total > INT32_MAX) {
        x.rc = MRT_ERR_TOO_LARGE;
        return x;
    }
    x.total = total;
    x.nb = ceil_div(total, blockRays);
    x.mine = (int)(x.nb > rank ? (x.nb - 1 - rank) / world + 1 : 0);   // <= nb <= total
    x.lastMine = x.mine > 0 && (x.nb - 1) % world == rank;
    x.numRays = (int64_t)x.mine * blockRays - (x.lastMine ? x.nb * blockRays - total : 0);
    return x;
}

OrderPlan plan_order(int mine, int order) {
    OrderPlan p;
    if (mine <= 0) return p;
    if (order == 0) {
        p.path = OrderPath::list;
        p.grid = grid_1d(mine);
        return p;
    }
    p.grid = grid_1d((int64_t)mine * 64);
    if (mine <= kOrderMax) {   // the list fits one workgroup's LDS: no scratch
        p.path = OrderPath::oneWorkgroup;
        return p;
    }
    p.path = OrderPath::tiled;
    p.numTiles = (int)ceil_div(mine, kOrderMax);   // <= 2^17
    p.tableWords = (int64_t)(kKeyMax + 1) * p.numTiles;
    p.scratchWords = p.tableWords + mine;          // < 2^30
    p.scratchBytes = (size_t)p.scratchWords * sizeof(int32_t);
    return p;
}

AOBlocksPlan plan_ao_blocks(int numInputRays, int numSamples, int numBatches, int batchInputRays, int numBlocks,
                            int blockRays, int64_t numOutRays) {
    AOBlocksPlan p;
    auto refuse = [&p](int rc, const char* why) {
        p.rc = rc;
        p.why = why;
        return p;
    };
    if (numInputRays < 0 || numSamples < 1 || numBlocks < 0 || blockRays < 1 || batchInputRays < 1 || numOutRays < 0)
        return refuse(MRT_ERR_INVALID_ARG, "bad ray/sample/block count");
    p.total = (int64_t)numInputRays * numSamples;
    if (p.total > INT32_MAX) return refuse(MRT_ERR_TOO_LARGE, "too many frame rays");
    p.needBatches = ceil_div(numInputRays, batchInputRays);
    if (numBatches < p.needBatches) return refuse(MRT_ERR_INVALID_ARG, "fewer batch seeds than batches");
    const int64_t nb = ceil_div(p.total, blockRays);
    if (numBlocks > nb) return refuse(MRT_ERR_INVALID_ARG, "more blocks listed than the frame has");
    // whole blocks, the last one listed perhaps short: ((numBlocks - 1) * B, numBlocks * B], or 0 of none
    if (numOutRays > (int64_t)numBlocks * blockRays || numOutRays < (int64_t)(numBlocks > 0 ? numBlocks - 1 : 0) * blockRays)
        return refuse(MRT_ERR_INVALID_ARG, "numOutRays does not match the listed blocks");
    p.empty = numOutRays == 0;
    // tiled: a workgroup's kTileRays outputs lie inside one block and hold whole input rays; the
    // tile's input rays and its sample points each fit one LDS slot per thread
    p.tiled = blockRays % kTileRays == 0 && kTileRays % numSamples == 0 && kTileRays / numSamples <= kThreads &&
              numSamples <= kThreads;
    p.grid = grid_1d(numOutRays, p.tiled ? kTileRays : kThreads);   // numOutRays <= nb * B < 2^32
    p.seedsInArgs = p.needBatches <= kMaxBatchSeeds;
    return p;
}

CountPlan plan_count(int numRays) {
    CountPlan c;
    // whole passes of a workgroup, at least one: kThreads <= perBlock <= 2^21
    const int64_t passes = ceil_div(ceil_div(numRays, kCountBlocks), kThreads);
    c.perBlock = (int)((passes > 0 ? passes : 1) * kThreads);
    c.blocks = (int)ceil_div(numRays, c.perBlock);
    return c;
}

}  // namespace mrt
