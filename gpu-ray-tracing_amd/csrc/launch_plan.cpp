// launch_plan.cpp — see launch_plan.hpp. No HIP here.
#include "launch_plan.hpp"

#include <algorithm>

#include "deal_common.hpp"
#include "trace_limits.hpp"
#include "tune.hpp"

namespace mrt {
namespace {

// LDS is handed out in granules; a total that is a multiple of this leaves no doubt about how
// a size is rounded (used where such a multiple lies inside the admissible range).
constexpr int kLdsRound = 2048;

// The production (speculative) traversal reads 4-wide nodes derived at bind time
// (profiles/round2_tuning.md, "4-wide nodes").
constexpr int kDefaultWide = 1;
// Launch schedules are tuned per batch size (tune.cpp): equal or faster on
// every workload once settled (+9...+16 % on bunny/dragon primary batches).
constexpr int kDefaultAutotune = 1;

// Rays per lane the automatic grid aims for: a frame-sized batch is bound by
// its slowest rays, whose step latency grows with the number of co-resident
// waves, so small batches get fewer waves per CU; big batches fill the CU.
// Measured on MI355X (tools/sweep.py, profiles/round1_sweep.txt): batches that
// fit one ray per lane at 32 waves/CU run fastest fully static (conference AO
// 640x480: 0.061 ms vs 0.077 at 8 waves); above that, 8 waves/CU is best up to
// ~1M rays (bunny primary 1024x768), 16 at 3M, 32 at 12M rays.
constexpr int kAutoRaysPerLane = 12;
constexpr int kAutoMinWaves = 8;

}  // namespace

mrt_launch_cfg default_cfg() {
    mrt_launch_cfg c{};
    c.waves_per_cu = 0;   // auto: sized from the batch (grid_waves_per_cu)
    c.fetch_threshold = 0;   // strided mode: a wave refills once all its lanes are done
    c.num_queues = -1;       // static strided assignment (see trace_kernel.hip); 1..8 = atomic queues
    c.lds_stack = 16;
    c.lane_groups = 1;
    c.wide = kDefaultWide;
    c.spec_slack = kDefaultSpecSlack;   // tune.hpp, like the tail: the autotuner changes them only at their defaults
    c.static_rounds = 1;
    c.autotune = kDefaultAutotune;
    c.tail_lanes = kDefaultTailLanes;
    c.queue_shared = 0;
    c.queue_block = 0;
    c.ray_sort = 0;
    c.queue_xcc_mask = 0;
    c.backfill = 0;          // the persistent grid
    c.oneshot = 0;           // the persistent kernels
    c.deal_block = 0;
    return c;
}

mrt_launch_cfg resolve_cfg(const mrt_launch_cfg& user) {
    mrt_launch_cfg c = user;
    const mrt_launch_cfg d = default_cfg();
    if (c.waves_per_cu == 0) c.waves_per_cu = d.waves_per_cu;
    if (c.num_queues == 0) c.num_queues = d.num_queues;
    if (c.lds_stack == 0) c.lds_stack = d.lds_stack;
    if (c.lane_groups == 0) c.lane_groups = d.lane_groups;
    if (c.wide < 0) c.wide = d.wide;   // -1 = library default
    if (c.spec_slack < 0) c.spec_slack = d.spec_slack;
    if (c.static_rounds == 0) c.static_rounds = d.static_rounds;
    if (c.autotune < 0) c.autotune = d.autotune;
    if (c.tail_lanes < 0) c.tail_lanes = d.tail_lanes;
    if (c.queue_shared < 0) c.queue_shared = d.queue_shared;
    if (c.queue_block < 0) c.queue_block = d.queue_block;
    if (c.queue_xcc_mask < 0) c.queue_xcc_mask = d.queue_xcc_mask;
    if (c.ray_sort < 0) c.ray_sort = d.ray_sort;
    if (c.backfill < 0) c.backfill = d.backfill;
    if (c.oneshot < 0) c.oneshot = d.oneshot;
    if (c.deal_block < 0) c.deal_block = d.deal_block;
    return c;
}

bool valid_cfg(const mrt_launch_cfg& c) {
    return (c.waves_per_cu == 0 || (c.waves_per_cu >= 4 && c.waves_per_cu <= 32)) && c.fetch_threshold >= 0 && c.fetch_threshold <= 64 &&
           (c.num_queues == -1 || (c.num_queues >= 1 && c.num_queues <= kMaxQueues)) &&
           (c.lds_stack == 8 || c.lds_stack == 16 || c.lds_stack == 32) &&
           c.lane_groups >= 1 && c.lane_groups <= 64 && (c.lane_groups & (c.lane_groups - 1)) == 0 &&
           (c.wide >= 0 && c.wide <= 2) && c.spec_slack >= 0 && c.spec_slack <= 63 &&
           c.static_rounds >= 1 && c.static_rounds <= 64 && (c.autotune == 0 || c.autotune == 1) &&
           c.tail_lanes >= 0 && c.tail_lanes <= 16 &&
           c.queue_shared >= 0 && c.queue_shared <= 100 && c.queue_block >= 0 && c.queue_block <= (1 << 20) &&
           (c.queue_block & (c.queue_block - 1)) == 0 && (c.queue_block == 0 || c.queue_block >= 64) &&
           c.queue_xcc_mask >= 0 && c.queue_xcc_mask <= 15 && (c.ray_sort == 0 || c.ray_sort == 1) &&
           c.backfill >= 0 && c.backfill <= kMaxBackfill &&
           // a backfilled grid is oversubscribed: only the static rounds, in which no workgroup waits for
           // another (the queues' unserved-queue sweep does), and not the one-round ray sort
           (c.backfill == 0 || (c.num_queues < 0 && c.ray_sort == 0)) &&
           // the one-shot kernels serve a grid of one ray per lane only (no queues and no ray sort: the
           // line above), and the deal's blocks are theirs
           (c.oneshot == 0 || (c.oneshot == 1 && c.backfill == 1)) &&
           (c.deal_block == 0 ||
            (c.oneshot == 1 && c.deal_block >= deal::kMinBlockLog2 && c.deal_block <= deal::kMaxBlockLog2));
}

int grid_waves_per_cu(int numCUs, const mrt_launch_cfg& cfg, int numRays) {
    int waves = cfg.waves_per_cu;
    if (waves == 0 && cfg.num_queues < 0) {
        // Static strided assignment: kStridedWaves per CU (tune.hpp).
        waves = kStridedWaves;
    } else if (waves == 0) {
        const long long cus = std::max(1, numCUs);
        if ((long long)numRays <= 32LL * 64 * cus) {
            // The whole batch fits the first (static, atomic-free) round at full
            // occupancy: one ray per lane, no dynamic fetch at all.
            waves = 32;
        } else {
            const long long lanesPerCU = (long long)numRays / kAutoRaysPerLane / cus;
            waves = (int)std::min<long long>(32, std::max<long long>(kAutoMinWaves, (lanesPerCU + 63) / 64));
        }
    }
    return waves;
}

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
