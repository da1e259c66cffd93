// launch_plan.hpp — the launch configuration (its defaults, the "library default" sentinels of
// mrt_tracer_set_config, its valid ranges and combinations, the waves per CU a batch gets) and
// the grid, the residency cap and the spill slab of a trace launch.
// Plain C++ with no HIP in it (like tune.hpp): mrt_api.cpp feeds it the caller's configuration,
// the device's and the kernel's figures, tests/cpp/launch_plan_driver.cpp runs it on the CPU.
//
// Two kinds of grid. The persistent one holds as many workgroups as are resident at once;
// each takes numRays / gridLanes static rounds. The backfilled one (cfg.backfill = k) is
// sized from the batch: every lane takes at most k rays, a workgroup ends after its k
// rounds and the hardware workgroup dispatcher starts the next one in the freed slot, so
// a tile of expensive rays holds its slot for its own duration only. How many workgroups
// share a CU is then no longer set by the grid; dynamic LDS passed at launch caps it.
//
// An oversubscribed grid must never run code in which one workgroup waits for another:
// the workgroup waited for may not be resident yet. The static strided rounds
// (num_queues = -1) have no such wait, and the plan is made for them only (valid_cfg
// refuses a backfill with queues or with the ray sort).
//
// A one-shot grid (cfg.oneshot, with backfill = 1) is the backfilled grid of the one-shot kernels:
// every lane at most one ray, dealt by deal_common.hpp in chunks of c positions per XCD group, so
// 8 * ceil(c / blockThreads) workgroups; with a block-cyclic deal c may exceed ceil(numRays / 8).
// Where it cannot be had (the batch fits the resident grid, or its slab exceeds the cap and would
// need more than one ray per lane) the plan is the one made without it, unchanged.
#pragma once

#include <cstdint>

#include "../../include/mrt.h"

namespace mrt {

// The configuration of a new tracer, and what a "library default" sentinel stands for.
mrt_launch_cfg default_cfg();
// The caller's configuration with every sentinel (0 for waves_per_cu, num_queues, lds_stack,
// lane_groups and static_rounds, negative for the fields after them) replaced by its default.
mrt_launch_cfg resolve_cfg(const mrt_launch_cfg& user);
// Whether a resolved configuration is one mrt_tracer_set_config accepts.
bool valid_cfg(const mrt_launch_cfg& c);
// Waves per CU a launch of numRays asks for on numCUs CUs: the configuration's, or what the
// batch size suggests.
int grid_waves_per_cu(int numCUs, const mrt_launch_cfg& cfg, int numRays);

constexpr int kMaxBackfill = 64;         // rays per lane a backfilled grid may be sized for
// Most bytes of a backfilled launch's spill slab, per workspace: the slab holds
// (stackCap - S) ints per launched lane, and a launched grid grows with the batch.
constexpr int64_t kSpillCapBytes = 256ll << 20;

struct LaunchPlanIn {
    int numRays = 0;
    int backfill = 0;        // 0: the persistent grid; 1..kMaxBackfill: rays per lane
    int numCUs = 1;
    int blockThreads = 256;  // threads per workgroup (trace_kernel.hpp kBlockThreads), a multiple of 64
    int wavesPerCU = 0;      // resident waves per CU asked for (> 0)
    int staticLds = 0;       // the kernel's static LDS bytes per workgroup
    int ldsPerCU = 0;        // LDS bytes of a CU
    int occBlocks = 1;       // workgroups per CU the code object admits without dynamic LDS
    int spillEntries = 0;    // stackCap - S: spill-slab ints per lane
    int64_t spillCapBytes = kSpillCapBytes;
    int oneshot = 0;         // 1: plan the one-shot grid (backfill == 1; the figures are the one-shot kernel's)
    int dealBlockLog2 = 0;   // its deal: 0 = contiguous chunks, 6..15 = 2^b-ray blocks dealt cyclically
};

struct LaunchPlan {
    int blocks = 0;          // workgroups launched
    int backfill = 0;        // rays per lane the grid was sized for (>= the asked k); 0: persistent
    int blocksPerCU = 0;     // workgroups resident per CU
    int dynLds = 0;          // dynamic LDS bytes per workgroup (the residency cap); 0: none needed
    int64_t spillInts = 0;   // spillEntries * launched lanes
    int oneshot = 0;         // 1: the one-shot grid was planned (else: the plan made without in.oneshot)
    int dealBlockLog2 = 0;   // its deal (0 when not one-shot)
};

// Workgroups per CU of a launch asked for wavesPerCU waves on a code object admitting occBlocks.
int plan_blocks_per_cu(int wavesPerCU, int occBlocks, int blockThreads = 256);
// Workgroups of a grid whose lanes take at most k rays each, a multiple of 8 (one XCD group each).
int64_t backfill_blocks(int64_t numRays, int k, int blockThreads = 256);
// Workgroups of the one-shot grid that deals numRays in 2^b-ray blocks (b = 0: contiguous chunks).
int64_t oneshot_blocks(int numRays, int dealBlockLog2, int blockThreads = 256);
// Dynamic LDS bytes with which exactly `blocks` workgroups of staticLds static bytes fit a CU's
// ldsPerCU; -1 when no size does (the static bytes alone admit fewer).
int cap_dyn_lds(int blocks, int staticLds, int ldsPerCU);
LaunchPlan plan_launch(const LaunchPlanIn& in);

}  // namespace mrt
