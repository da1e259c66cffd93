// launch_plan.cpp — see launch_plan.hpp. No HIP here.
#include "launch_plan.hpp"

#include <algorithm>

#include "deal_common.hpp"

namespace mrt {
namespace {

// LDS is handed out in granules; a total that is a multiple of this leaves no doubt about how
// a size is rounded (used where such a multiple lies inside the admissible range).
constexpr int kLdsRound = 2048;

}  // namespace

int plan_blocks_per_cu(int wavesPerCU, int occBlocks, int blockThreads) {
    const int wavesPerBlock = std::max(1, blockThreads / 64);
    const int want = std::max(1, (wavesPerCU + wavesPerBlock - 1) / wavesPerBlock);
    return std::min(want, std::max(1, occBlocks));
}

int64_t backfill_blocks(int64_t numRays, int k, int blockThreads) {
    const int64_t lanes = (numRays + k - 1) / k;
    const int64_t blocks = (lanes + blockThreads - 1) / blockThreads;
    return (blocks + 7) / 8 * 8;
}

int64_t oneshot_blocks(int numRays, int dealBlockLog2, int blockThreads) {
    const int c = deal::chunk(numRays, dealBlockLog2);
    return (int64_t)deal::kGroups * deal::blocks_per_group(c, blockThreads);
}

int cap_dyn_lds(int blocks, int staticLds, int ldsPerCU) {
    if (blocks < 1 || staticLds < 0 || ldsPerCU <= 0) return -1;
    // exactly `blocks` fit when the bytes per workgroup T satisfy L / (blocks + 1) < T <= L / blocks
    const int hi = ldsPerCU / blocks;
    const int lo = ldsPerCU / (blocks + 1);   // T must exceed this
    if (staticLds > hi) return -1;
    if (staticLds > lo) return 0;             // the static bytes alone admit exactly `blocks`
    const int rounded = hi / kLdsRound * kLdsRound;
    const int total = rounded > lo ? rounded : hi;
    return total - staticLds;
}

LaunchPlan plan_launch(const LaunchPlanIn& in) {
    LaunchPlan p;
    const int perCU = plan_blocks_per_cu(in.wavesPerCU, in.occBlocks, in.blockThreads);
    const int64_t resident = (int64_t)perCU * std::max(1, in.numCUs);
    const int64_t entries = std::max(0, in.spillEntries);
    // the persistent plan, as it has always been: every workgroup resident for the whole launch
    p.blocks = (int)resident;
    p.backfill = 0;
    p.blocksPerCU = perCU;
    p.dynLds = 0;
    p.spillInts = entries * resident * in.blockThreads;
    if (in.backfill <= 0 || in.numRays <= 0) return p;

    // The one-shot grid: only when the batch does not fit the resident grid (then there is nothing
    // to backfill) and the slab of its launched lanes fits the cap (else k > 1: not one-shot).
    if (in.oneshot == 1 && in.backfill == 1 && (in.dealBlockLog2 == 0 || (in.dealBlockLog2 >= deal::kMinBlockLog2 &&
                                                                          in.dealBlockLog2 <= deal::kMaxBlockLog2)) &&
        backfill_blocks(in.numRays, 1, in.blockThreads) > resident) {
        const int64_t blocks = oneshot_blocks(in.numRays, in.dealBlockLog2, in.blockThreads);
        const int64_t spillInts = entries * blocks * in.blockThreads;
        int dyn = 0;
        if (perCU < in.occBlocks) dyn = cap_dyn_lds(perCU, in.staticLds, in.ldsPerCU);
        if (spillInts * (int64_t)sizeof(int32_t) <= in.spillCapBytes && dyn >= 0 && blocks * in.blockThreads <= 0x7fffffffll) {
            p.blocks = (int)blocks;
            p.backfill = 1;
            p.dynLds = dyn;
            p.spillInts = spillInts;
            p.oneshot = 1;
            p.dealBlockLog2 = in.dealBlockLog2;
            return p;
        }
    }

    // The smallest k from the asked one whose slab fits the cap: the slab is indexed by the
    // launched lane, so it grows with the grid, and a larger k is a smaller grid.
    for (int k = std::min(in.backfill, kMaxBackfill); k <= kMaxBackfill; k++) {
        const int64_t blocks = backfill_blocks(in.numRays, k, in.blockThreads);
        if (blocks <= resident) return p;   // the batch fits the resident grid: nothing to backfill
        const int64_t spillInts = entries * blocks * in.blockThreads;
        if (spillInts * (int64_t)sizeof(int32_t) > in.spillCapBytes) continue;
        int dyn = 0;
        if (perCU < in.occBlocks) {
            dyn = cap_dyn_lds(perCU, in.staticLds, in.ldsPerCU);
            if (dyn < 0) return p;          // no LDS size gives this residency: never launch at an unknown one
        }
        p.blocks = (int)blocks;
        p.backfill = k;
        p.dynLds = dyn;
        p.spillInts = spillInts;
        return p;
    }
    return p;   // no k up to kMaxBackfill fits the slab: the persistent grid
}

}  // namespace mrt
