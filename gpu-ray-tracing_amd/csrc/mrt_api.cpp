// mrt_api.cpp — the C-ABI of include/mrt.h: per-device tracer contexts, the
// persistent-grid sizing, the workspace (queue heads, stack spill slab) and the
// events that time the autotuner's launches (its policy: tune.cpp; the
// reference-compatible entry points of CudaTracerKernels.hh:42-52: compat_api.cpp).
//
// The library never owns the caller's BVH/ray/result buffers (reference
// ownership: CudaBVH.cc:101-109, RayBuffer.cc:42-81). It owns only its
// workspace, sized for the persistent grid it launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mrt.h"
#include "deal_common.hpp"
#include "lbvh_common.hpp"
#include "launch_plan.hpp"
#include "lbvh_kernel.hpp"
#include "refit_kernel.hpp"
#include "refit_plan.hpp"
#include "trace_kernel.hpp"
#include "tune.hpp"

namespace mrt {
struct Workspace;
static_assert(kTuneMaxQueues == kMaxQueues, "the per-XCD queue candidate's queue count");
// The event pairs of a TuneState's timing slots (created lazily, destroyed in tune_reset).
struct TuneEvents {
    hipEvent_t start[TuneState::kSlots] = {}, stop[TuneState::kSlots] = {};
};
}

struct mrt_tracer {
    int device = 0;
    int numCUs = 0;
    int numXccs = 1;   // XCDs of the device (partition): the per-XCD queue candidate's queue count
    int ldsPerCU = 0;  // LDS bytes of a CU (the device attribute; 0: unknown, no backfilled launches)
    int ldsPerBlock = 0;   // most LDS bytes one workgroup may hold
    std::mutex mu;

    // Bound Compact2 BVH (borrowed device pointers).
    bool bound = false;
    const void* nodes = nullptr;
    int64_t nodeBytes = 0;
    const void* woop = nullptr;
    int64_t woopBytes = 0;
    const int32_t* triIndex = nullptr;
    int64_t triIndexBytes = 0;

    mrt_launch_cfg cfg{};

    // 4-wide nodes derived from the bound Compact2 tree (cfg.wide; wide_bvh.cpp),
    // owned by the tracer and rebuilt when the BVH or the setting changes.
    void* wideNodes = nullptr;
    int64_t wideBytes = 0;
    int wideBuiltFor = -1;   // the cfg.wide value the current array was built for
    int wideFormat = mrt::kNodeCompact2;   // the form wideNodes holds (kNodeWide4 / kNodeWide4Q)
    bool wideLeafCounts = false;           // its leaf refs carry triangle counts
    // Stack entries (sentinel included) the wide traversal gets: the wide tree's
    // worst case (wide_stack_bound) + 1, at least the reference's 64. A wide node
    // pushes up to three children where the binary step pushes one, so a tree that
    // fits the reference's stack in binary order could otherwise overflow in wide
    // order; sized this way no ray of the bound tree can overflow it.
    int wideStackCap = mrt::kStackCapacity;
    int wideStackBound = mrt::kStackCapacity - 1;   // wide_stack_bound of the derived tree (the tail's headroom)
    double bindMs = 0.0;                   // wall time of the last bind / wide derivation (mrt_trace_info)
    // Exact form only: per wide child the Compact2 slot (binary node * 2 + side) its box was
    // copied from, -1 = absent — from the collapse that produced wideNodes (a refit copies the
    // refitted boxes along it; collapsing refitted nodes again would choose other children).
    std::vector<int32_t> wideSrc;

    // The refit plan (mrt_tracer_refit), built on the first refit after a bind or set_config
    // and dropped by bind, unbind and set_config: the nodes by height level, the wide source
    // map and the refit's scratch, on the device.
    bool planBuilt = false;
    int32_t* planOrder = nullptr;      // numNodes node indices, level by level
    int32_t* planOffsets = nullptr;    // levels + 1 offsets into planOrder
    int32_t* planWideSrc = nullptr;    // wideSrc on the device (null: no exact wide array)
    uint8_t* planValid = nullptr;      // 2 per node, rewritten by every refit
    unsigned long long* planSkipped = nullptr;   // out-of-range references skipped since the last refit_info
    std::vector<int64_t> planLevels;   // the level offsets on the host
    int64_t planBytes = 0;
    int refitLaunches = 0;             // kernel launches of the last refit
    bool refitLaunched = false;        // a refit may still be running

    mrt_build_info lastBuild{};        // the last successful mrt_tracer_build (mrt_tracer_build_info)

    // Launch scratch, one set per stream the handle has launched on: the stack
    // spill slab, the queue heads and the overflow counter are written by a
    // running trace, so two traces in flight on different streams must not
    // share them (the handle's mutex only covers enqueueing).
    std::vector<mrt::Workspace*> workspaces;
    uint64_t useClock = 0;   // launches of this handle (the workspaces' LRU order; guarded by mu)
    hipEvent_t evStart = nullptr, evStop = nullptr;

    // Occupancy per kernel (index kernel_key(), below 1024), queried once
    // (hipOccupancy* is a host round-trip that would otherwise sit on every launch).
    int occ[1024] = {};
    // Backfilled launches (launch_plan.hpp): per variant and residency cap of 1..kMaxCapBlocks
    // workgroups per CU, the dynamic LDS bytes + 1 that the occupancy query confirmed to give
    // exactly that residency (0: not asked yet, -1: none found, such launches run persistent).
    static constexpr int kMaxCapBlocks = 8;
    int capDyn[1024][kMaxCapBlocks + 1] = {};
    int staticLds[1024] = {};   // per kernel: its static LDS bytes + 1 (0: not asked yet)

    // cfg.autotune: per (batch size, variant) the ray-distribution schedule the
    // measured launches chose (tune.cpp), reset on bind/set_config.
    mrt::TuneTable tunes;
};

namespace mrt {
namespace {
thread_local std::string g_lastError;
}  // namespace

// Shared with the ray-generation entry points (csrc/raygen_kernel.hip).
int api_fail(int code, const std::string& what) {
    g_lastError = what;
    return code;
}
const char* api_last_error() { return g_lastError.c_str(); }

struct Workspace {
    void* stream = nullptr;       // the hipStream_t this scratch was last used on
    unsigned* queues = nullptr;   // kMaxQueues * kQueueStrideWords words
    int* status = nullptr;        // [0] = stack overflows of asynchronous launches since the last reset
                                  // (sticky); [kTimedSlot] = the current blocking launch's own count
    int* spill = nullptr;
    size_t spillInts = 0;
    // -DMRT_DONE_EVENT: recorded after every launch that uses this scratch, so waiting
    // for it never touches the stream (see workspace_wait)
    hipEvent_t done = nullptr;
    bool launched = false;        // a launch may still be using this scratch
    uint64_t lastUse = 0;         // launch counter value of the last use (LRU reuse)
};
constexpr int kTimedSlot = 16;    // a separate 64-B line of Workspace::status
// The per-launch completion event only tells the host that the launch has finished
// (workspace reuse, destroy, overflow reads): no system-scope fence, which would
// write back and invalidate the caches between back-to-back launches.
#ifdef MRT_DONE_EVENT
#ifndef MRT_DONE_EVENT_FLAGS
#define MRT_DONE_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#endif
constexpr unsigned kDoneEventFlags = MRT_DONE_EVENT_FLAGS;
#endif
// Events that only time launches (the autotuner's, the blocking call's start).
#ifndef MRT_TIMING_EVENT_FLAGS
#define MRT_TIMING_EVENT_FLAGS hipEventDisableSystemFence
#endif
constexpr unsigned kTimingEventFlags = MRT_TIMING_EVENT_FLAGS;
// Scratch sets per handle: a trace on a new stream reuses the least recently used
// set (after its last launch has completed) once this many exist.
constexpr int kMaxWorkspaces = 8;
}  // namespace mrt

namespace {

int fail(int code, const std::string& what) { return mrt::api_fail(code, what); }

int hipFail(hipError_t e, const char* what) {
    return fail(MRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define MRT_HIP(call)                                  \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hipFail(e_, #call); \
    } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// The production (speculative) traversal reads 4-wide nodes derived at bind time
// (profiles/round2_tuning.md, "4-wide nodes").
constexpr int kDefaultWide = 1;
// Launch schedules are tuned per batch size (tune.cpp): equal or faster on
// every workload once settled (+9...+16 % on bunny/dragon primary batches).
constexpr int kDefaultAutotune = 1;

mrt_launch_cfg default_cfg() {
    mrt_launch_cfg c;
    c.waves_per_cu = 0;   // auto: sized from the batch (grid_waves_per_cu)
    c.fetch_threshold = 0;   // strided mode: a wave refills once all its lanes are done
    c.num_queues = -1;       // static strided assignment (see trace_kernel.hip); 1..8 = atomic queues
    c.lds_stack = 16;
    c.lane_groups = 1;
    c.wide = kDefaultWide;
    c.spec_slack = mrt::kDefaultSpecSlack;   // tune.hpp, like the tail: the autotuner changes them only at their defaults
    c.static_rounds = 1;
    c.autotune = kDefaultAutotune;
    c.tail_lanes = mrt::kDefaultTailLanes;
    c.queue_shared = 0;
    c.queue_block = 0;
    c.ray_sort = 0;
    c.queue_xcc_mask = 0;
    c.backfill = 0;          // the persistent grid
    c.oneshot = 0;           // the persistent kernels
    c.deal_block = 0;
    return c;
}

bool valid_cfg(const mrt_launch_cfg& c) {
    return (c.waves_per_cu == 0 || (c.waves_per_cu >= 4 && c.waves_per_cu <= 32)) && c.fetch_threshold >= 0 && c.fetch_threshold <= 64 &&
           (c.num_queues == -1 || (c.num_queues >= 1 && c.num_queues <= mrt::kMaxQueues)) &&
           (c.lds_stack == 8 || c.lds_stack == 16 || c.lds_stack == 32) &&
           c.lane_groups >= 1 && c.lane_groups <= 64 && (c.lane_groups & (c.lane_groups - 1)) == 0 &&
           (c.wide >= 0 && c.wide <= 2) && c.spec_slack >= 0 && c.spec_slack <= 63 &&
           c.static_rounds >= 1 && c.static_rounds <= 64 && (c.autotune == 0 || c.autotune == 1) &&
           c.tail_lanes >= 0 && c.tail_lanes <= 16 &&
           c.queue_shared >= 0 && c.queue_shared <= 100 && c.queue_block >= 0 && c.queue_block <= (1 << 20) &&
           (c.queue_block & (c.queue_block - 1)) == 0 && (c.queue_block == 0 || c.queue_block >= 64) &&
           c.queue_xcc_mask >= 0 && c.queue_xcc_mask <= 15 && (c.ray_sort == 0 || c.ray_sort == 1) &&
           c.backfill >= 0 && c.backfill <= mrt::kMaxBackfill &&
           // a backfilled grid is oversubscribed: only the static rounds, in which no workgroup waits for
           // another (the queues' unserved-queue sweep does), and not the one-round ray sort
           (c.backfill == 0 || (c.num_queues < 0 && c.ray_sort == 0)) &&
           // the one-shot kernels serve a grid of one ray per lane only (no queues and no ray sort: the
           // line above), and the deal's blocks are theirs
           (c.oneshot == 0 || (c.oneshot == 1 && c.backfill == 1)) &&
           (c.deal_block == 0 ||
            (c.oneshot == 1 && c.deal_block >= mrt::deal::kMinBlockLog2 && c.deal_block <= mrt::deal::kMaxBlockLog2));
}

// The frontier tail runs in the exact 4-wide kernels whose leaf refs carry counts.
bool with_tail(const mrt_tracer* t, const mrt::TraceVariant& v, const mrt_launch_cfg& c) {
    return c.tail_lanes > 0 && v.nodes == mrt::kNodeWide4 && t->wideLeafCounts;
}

mrt::TraceVariant variant_for(const mrt_tracer* t, uint32_t flags) {
    mrt::TraceVariant v;
    v.anyHit = (flags & MRT_TRACE_ANY_HIT) != 0;
    v.exactRcp = (flags & MRT_TRACE_EXACT_RCP) != 0;
    v.speculative = (flags & MRT_TRACE_LOCKSTEP_OFF) == 0;
    v.stats = (flags & MRT_TRACE_STATS) != 0;
    v.ldsStack = t->cfg.lds_stack;
    // The per-lane (lockstep-off) order is the reference's binary order: it keeps
    // the Compact2 nodes, and with them the oracle's exact per-ray counters.
    v.nodes = (t->cfg.wide != 0 && t->wideNodes != nullptr && v.speculative) ? t->wideFormat : mrt::kNodeCompact2;
    v.tail = with_tail(t, v, t->cfg);
    return v;
}

// Rays per lane the automatic grid aims for: a frame-sized batch is bound by
// its slowest rays, whose step latency grows with the number of co-resident
// waves, so small batches get fewer waves per CU; big batches fill the CU.
// Measured on MI355X (tools/sweep.py, profiles/round1_sweep.txt): batches that
// fit one ray per lane at 32 waves/CU run fastest fully static (conference AO
// 640x480: 0.061 ms vs 0.077 at 8 waves); above that, 8 waves/CU is best up to
// ~1M rays (bunny primary 1024x768), 16 at 3M, 32 at 12M rays.
constexpr int kAutoRaysPerLane = 12;
constexpr int kAutoMinWaves = 8;

// The key of a kernel variant: its part of the tuning key (a saved schedule's one-shot bits are
// part of the schedule, not of the key).
int variant_key(const mrt::TraceVariant& v) {
    const int lds = v.ldsStack == 8 ? 0 : v.ldsStack == 16 ? 1 : 2;
    return (v.anyHit ? 1 : 0) | (v.speculative ? 2 : 0) | (v.exactRcp ? 4 : 0) | (v.stats ? 8 : 0) | (lds << 4) |
           (v.nodes << 6) | (v.tail ? 256 : 0);   // < 512
}

// The key of a kernel function: its slot in mrt_tracer::occ, capDyn and staticLds (a variant's
// one-shot sibling is a function of its own: other registers, less static LDS).
int kernel_key(const mrt::TraceVariant& v) {
    static_assert((15 | (2 << 4) | (mrt::kNodeWide4Q << 6) | (1 << 8) | (1 << 9)) < (int)(sizeof(mrt_tracer::occ) / sizeof(int)),
                  "every kernel_key indexes mrt_tracer::occ");
    return variant_key(v) | (v.oneshot ? 512 : 0);
}

// Workgroups per CU the code object of a variant admits (queried once).
int variant_occupancy(mrt_tracer* t, const mrt::TraceVariant& v) {
    int& occ = t->occ[kernel_key(v)];
    if (occ <= 0 && (mrt::trace_occupancy(v, &occ) != hipSuccess || occ <= 0)) occ = 1;
    return occ;
}

// Waves per CU a launch asks for: the configuration's, or what the batch size suggests.
int grid_waves_per_cu(const mrt_tracer* t, const mrt_launch_cfg& cfg, int numRays) {
    int waves = cfg.waves_per_cu;
    if (waves == 0 && cfg.num_queues < 0) {
        // Static strided assignment: 28 waves/CU (7 workgroups) measured best or
        // within 2 % of best from 307k to 12.6M rays (profiles/round1_sweep.txt).
        waves = mrt::kStridedWaves;
    } else if (waves == 0) {
        const long long cus = std::max(1, t->numCUs);
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

static_assert(mrt::kTuneMaxBackfill == mrt::kMaxBackfill, "tune.hpp restates launch_plan.hpp's kMaxBackfill");
static_assert(mrt::TuneState::kTuneMinDealBlock == mrt::deal::kMinBlockLog2 &&
                  mrt::TuneState::kTuneMaxDealBlock == mrt::deal::kMaxBlockLog2,
              "tune.hpp restates deal_common.hpp's block range");

// The dynamic LDS with which exactly perCU workgroups of variant v are resident per CU, confirmed
// by the occupancy query once per (variant, perCU); -1 when no size is confirmed. The arithmetic
// (cap_dyn_lds) proposes, the query decides: a disagreement is repaired by stepping the size, and
// a launch never runs at a residency nobody confirmed.
int confirmed_cap_lds(mrt_tracer* t, const mrt::TraceVariant& v, int perCU, int staticLds, int proposed) {
    if (perCU < 1 || perCU > mrt_tracer::kMaxCapBlocks) return -1;
    int& slot = t->capDyn[kernel_key(v)][perCU];
    if (slot != 0) return slot > 0 ? slot - 1 : -1;
    slot = -1;
    constexpr int kStep = 1024, kMaxSteps = 32;
    int dyn = proposed;
    for (int i = 0; i < kMaxSteps && dyn >= 0 && staticLds + dyn <= std::min(t->ldsPerCU, t->ldsPerBlock); i++) {
        // above 64 KB a launch needs the function's dynamic-LDS limit raised first
        if (staticLds + dyn > (64 << 10) && mrt::trace_allow_dynamic_lds(v, dyn) != hipSuccess) break;
        int got = 0;
        if (mrt::trace_occupancy(v, &got, dyn) != hipSuccess) break;
        if (got == perCU) {
            slot = dyn + 1;
            return dyn;
        }
        dyn += got > perCU ? kStep : -kStep;
    }
    (void)hipGetLastError();   // a refused query leaves no sticky error behind
    return -1;
}

// The launch's grid (launch_plan.hpp): the persistent one — as many 256-thread workgroups per CU
// as the config asks for (or the batch size suggests) and the code object's occupancy admits,
// every workgroup resident at once — or, with cfg.backfill, one sized from the batch.
mrt::LaunchPlan launch_plan(mrt_tracer* t, const mrt_launch_cfg& cfg, const mrt::TraceVariant& v, int numRays, int stackCap) {
    mrt::LaunchPlanIn in;
    in.numRays = numRays;
    in.numCUs = t->numCUs;
    in.blockThreads = mrt::kBlockThreads;
    in.wavesPerCU = grid_waves_per_cu(t, cfg, numRays);
    in.occBlocks = variant_occupancy(t, v);
    in.spillEntries = stackCap - v.ldsStack;
    in.ldsPerCU = t->ldsPerCU;
    mrt::LaunchPlan persistent = mrt::plan_launch(in);
    if (cfg.backfill <= 0 || cfg.num_queues >= 1 || t->ldsPerCU <= 0) return persistent;
    int& lds = t->staticLds[kernel_key(v)];
    if (lds == 0) {   // from the function's attributes, once per variant (a host round trip)
        hipFuncAttributes attr{};
        if (mrt::trace_kernel_attributes(v, &attr) != hipSuccess) return persistent;
        lds = (int)attr.sharedSizeBytes + 1;
    }
    in.backfill = cfg.backfill;
    in.oneshot = v.oneshot ? 1 : 0;   // the plan of the one-shot kernel, from its own occupancy and static LDS
    in.dealBlockLog2 = cfg.deal_block;
    in.staticLds = lds - 1;
    mrt::LaunchPlan p = mrt::plan_launch(in);
    if (p.backfill > 0 && p.dynLds > 0) {
        const int dyn = confirmed_cap_lds(t, v, p.blocksPerCU, in.staticLds, p.dynLds);
        if (dyn < 0) return persistent;
        p.dynLds = dyn;
    }
    return p;
}

// Waits for the last launch that used `w` without touching the stream it ran on (the
// caller may have destroyed it): a device-wide synchronize. A completion event recorded
// after every launch (-DMRT_DONE_EVENT) would let the wait cover this handle's launches
// only, but an event between back-to-back launches costs each of them 1-3 % (measured:
// conference AO 0.0352 -> 0.0361 ms, bunny 640x480 0.0945 -> 0.0959 ms,
// profiles/round3_tuning.md); the waits are rare (bind, set_config, destroy, overflow
// reads, a ninth stream).
int workspace_wait(mrt::Workspace* w) {
    if (!w->launched) return MRT_OK;
#ifdef MRT_DONE_EVENT
    MRT_HIP(hipEventSynchronize(w->done));
#else
    MRT_HIP(hipDeviceSynchronize());
    w->launched = false;
#endif
    return MRT_OK;
}

// Every launch of this handle has completed (bind, set_config and destroy).
int wait_all_workspaces(mrt_tracer* t) {
    for (mrt::Workspace* w : t->workspaces)
        if (int rc = workspace_wait(w)) return rc;
    return MRT_OK;
}

// The scratch of `stream`: its own set, else a new one, else (kMaxWorkspaces
// reached) the least recently used set once its last launch has completed —
// grown to the grid's spill slab.
int workspace_for(mrt_tracer* t, void* stream, int totalLanes, int ldsStack, int stackCap, mrt::Workspace** out) {
    mrt::Workspace* w = nullptr;
    for (mrt::Workspace* x : t->workspaces)
        if (x->stream == stream) w = x;
    if (!w && (int)t->workspaces.size() >= mrt::kMaxWorkspaces) {
        for (mrt::Workspace* x : t->workspaces)
            if (!w || x->lastUse < w->lastUse) w = x;
        if (int rc = workspace_wait(w)) return rc;   // its previous stream's launch may still run
        w->stream = stream;
    }
    if (!w) {
        w = new mrt::Workspace();
        w->stream = stream;
        t->workspaces.push_back(w);
        MRT_HIP(hipMalloc(&w->queues, mrt::kQueueLines * mrt::kQueueStrideWords * sizeof(unsigned)));
        MRT_HIP(hipMalloc(&w->status, 64 * sizeof(int)));
        MRT_HIP(hipMemset(w->status, 0, 64 * sizeof(int)));
#ifdef MRT_DONE_EVENT
        MRT_HIP(hipEventCreateWithFlags(&w->done, mrt::kDoneEventFlags));
#endif
    }
    w->lastUse = ++t->useClock;
    const size_t need = (size_t)(stackCap - ldsStack) * (size_t)totalLanes;
    if (need > w->spillInts) {
        // A smaller slab may still be in use by this scratch's previous launch.
        if (int rc = workspace_wait(w)) return rc;
        if (w->spill) MRT_HIP(hipFree(w->spill));
        w->spill = nullptr;
        w->spillInts = 0;
        MRT_HIP(hipMalloc(&w->spill, need * sizeof(int)));
        w->spillInts = need;
    }
    if (!t->evStart) {
        // the blocking call's timing pair: no system-scope fence around the kernel (it would
        // flush the caches and be timed with it); the stop event releases to device scope,
        // so the overflow count read after it is current
        MRT_HIP(hipEventCreateWithFlags(&t->evStart, mrt::kTimingEventFlags));
        MRT_HIP(hipEventCreateWithFlags(&t->evStop, hipEventReleaseToDevice));
    }
    *out = w;
    return MRT_OK;
}

// Forgets the refit plan (bind, unbind, set_config, destroy; the handle's mutex held).
void drop_plan(mrt_tracer* t) {
    if (t->refitLaunched) (void)hipDeviceSynchronize();   // a refit may still read the plan
    t->refitLaunched = false;
    for (void* p : {(void*)t->planOrder, (void*)t->planOffsets, (void*)t->planWideSrc, (void*)t->planValid,
                    (void*)t->planSkipped})
        if (p) (void)hipFree(p);
    t->planOrder = t->planOffsets = t->planWideSrc = nullptr;
    t->planValid = nullptr;
    t->planSkipped = nullptr;
    t->planLevels.clear();
    t->planBytes = 0;
    t->planBuilt = false;
    t->refitLaunches = 0;
}

// Largest wide-traversal stack a tracer sizes its spill slab for (entries per lane).
constexpr int kMaxWideStack = 1024;

// (Re)derives the 4-wide nodes of the bound BVH when cfg.wide asks for them;
// bind, unbind and set_config call it with the handle's mutex held. Synchronous
// (bind-time work: the Compact2 nodes come to the host, collapse, go back).
int refresh_wide(mrt_tracer* t) {
    const int want = t->bound ? t->cfg.wide : 0;
    if (want == t->wideBuiltFor) return MRT_OK;
    DeviceGuard guard(t->device);
    // launches in flight may still read the old array: wait for this handle's own
    if (int rc = wait_all_workspaces(t)) return rc;
    if (t->refitLaunched) MRT_HIP(hipDeviceSynchronize());   // a refit's gather may still write it
    t->refitLaunched = false;
    if (t->wideNodes) MRT_HIP(hipFree(t->wideNodes));
    t->wideNodes = nullptr;
    t->wideBytes = 0;
    t->wideBuiltFor = -1;
    t->wideFormat = mrt::kNodeCompact2;
    t->wideStackCap = mrt::kStackCapacity;
    t->wideStackBound = mrt::kStackCapacity - 1;
    t->wideSrc.clear();
    if (want) {
        std::vector<int32_t> host((size_t)(t->nodeBytes / 4));
        MRT_HIP(hipMemcpy(host.data(), t->nodes, (size_t)t->nodeBytes, hipMemcpyDeviceToHost));
        // The first word of every Woop slot (the terminators): the leaf refs carry counts.
        const int64_t slots = t->woopBytes / 16;
        const bool counts = mrt::leaf_counts_fit(slots);
        std::vector<int32_t> woopX;
        if (counts) {
            woopX.resize((size_t)slots);
            MRT_HIP(hipMemcpy2D(woopX.data(), 4, t->woop, 16, 4, (size_t)slots, hipMemcpyDeviceToHost));
        }
        const int32_t* wx = counts ? woopX.data() : nullptr;
        std::vector<uint32_t> wide;
        int format = mrt::kNodeWide4;
        // The quantized form when asked for and every box quantizes; else the exact one.
        if (want == 2 && mrt::build_wide4q(host.data(), t->nodeBytes / 64, &wide, wx, slots)) format = mrt::kNodeWide4Q;
        else wide = mrt::build_wide4(host.data(), t->nodeBytes / 64, wx, slots, &t->wideSrc);
        t->wideLeafCounts = counts;
        const int nodeWords = format == mrt::kNodeWide4 ? 32 : 16;
        const int64_t need = mrt::wide_stack_bound(wide.data(), (int64_t)wide.size() / nodeWords, nodeWords);
        if (need + 1 > kMaxWideStack) {   // a degenerate tree: keep the binary traversal and its reference capacity
            t->wideBuiltFor = want;
            return MRT_OK;
        }
        t->wideStackCap = std::max<int>(mrt::kStackCapacity, (int)need + 1);
        t->wideStackBound = (int)need;
        const int64_t bytes = (int64_t)wide.size() * 4;
        if (bytes > mrt::kMaxBufferBytes) return fail(MRT_ERR_TOO_LARGE, "4-wide node array above the 32-bit range");
        MRT_HIP(hipMalloc(&t->wideNodes, (size_t)bytes));
        MRT_HIP(hipMemcpy(t->wideNodes, wide.data(), (size_t)bytes, hipMemcpyHostToDevice));
        t->wideBytes = bytes;
        t->wideFormat = format;
    }
    t->wideBuiltFor = want;
    return MRT_OK;
}

// ---- launch-schedule autotuning (cfg.autotune): the events ----------------------
// The policy is tune.cpp's (the candidate table tune_candidate, the stages, the table of
// settled schedules); here are the event pairs that time its exploring launches.

// Feeds the timings of the launches that have completed to their state (never blocking).
void tune_collect(mrt::TuneState* st) {
    for (int s = 0; s < mrt::TuneState::kSlots; s++) {
        if (st->slotCand[s] < 0 || hipEventQuery(st->events->stop[s]) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, st->events->start[s], st->events->stop[s]) == hipSuccess) st->slot_done(s, ms);
        else st->slot_dropped(s);
    }
}

// The event pair of timing slot `slot`, created on its first use.
int tune_events(mrt::TuneState* st, int slot, hipEvent_t* start, hipEvent_t* stop) {
    if (!st->events) st->events = new mrt::TuneEvents();
    mrt::TuneEvents* ev = st->events;
    if (!ev->start[slot]) {
        MRT_HIP(hipEventCreateWithFlags(&ev->start[slot], mrt::kTimingEventFlags));
        MRT_HIP(hipEventCreateWithFlags(&ev->stop[slot], mrt::kTimingEventFlags));
    }
    *start = ev->start[slot];
    *stop = ev->stop[slot];
    return MRT_OK;
}

void tune_reset(mrt_tracer* t) {
    for (auto& kv : t->tunes.tunes) {
        mrt::TuneEvents* ev = kv.second->events;
        for (int s = 0; ev && s < mrt::TuneState::kSlots; s++) {
            if (ev->start[s]) (void)hipEventSynchronize(ev->stop[s]);
            if (ev->start[s]) (void)hipEventDestroy(ev->start[s]);
            if (ev->stop[s]) (void)hipEventDestroy(ev->stop[s]);
        }
        delete ev;
    }
    t->tunes.clear();
}

// The bind itself, arguments checked and the handle's mutex held (mrt_tracer_bind, mrt_tracer_build).
int bind_locked(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                const int32_t* triIndex, int64_t triIndexBytes) {
    t->nodes = nodes;
    t->nodeBytes = nodeBytes;
    t->woop = woop;
    t->woopBytes = woopBytes;
    t->triIndex = triIndex;
    t->triIndexBytes = triIndexBytes;
    t->bound = true;
    t->wideBuiltFor = -1;   // a new BVH: its wide nodes are derived now (if configured)
    DeviceGuard guard(t->device);
    tune_reset(t);          // and its schedules are tuned again
    drop_plan(t);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = refresh_wide(t);
    t->bindMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// Largest batch one launch takes: ray/result addressing and the strided round
// arithmetic stay inside int32 with room for the grid (bigger batches are split
// by the caller, as the reference Renderer does at 2^21 rays, Renderer.cc:46).
constexpr int32_t kMaxRaysPerLaunch = 1 << 30;

// The checks of a trace call that need no look at the handle's state, and (with its mutex
// held, for a batch that is not empty) those of the batch against the bound BVH.
int check_call(const mrt_tracer* t, int32_t numRays, uint32_t flags) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    if (numRays < 0) return fail(MRT_ERR_INVALID_ARG, "numRays < 0");
    if (flags & ~0x1Fu) return fail(MRT_ERR_INVALID_ARG, "unknown trace flag");
    return MRT_OK;
}

int check_batch(const mrt_tracer* t, const void* rays, const void* results, int32_t numRays, uint32_t flags,
                const int32_t* stats) {
    if (!t->bound) return fail(MRT_ERR_NOT_BOUND, "trace before bind (no BVH)");
    if (!rays || !results) return fail(MRT_ERR_INVALID_ARG, "null ray/result buffer");
    if ((flags & MRT_TRACE_STATS) && !stats) return fail(MRT_ERR_INVALID_ARG, "MRT_TRACE_STATS without stats buffer");
    if (numRays > kMaxRaysPerLaunch) return fail(MRT_ERR_TOO_LARGE, "more than 2^30 rays in one launch: split the batch");
    return MRT_OK;
}

// The kernel arguments of a launch of `totalLanes` lanes with configuration cfg on scratch ws;
// the caller adds the rays, results and stats buffers.
mrt::TraceArgs trace_args(const mrt_tracer* t, const mrt_launch_cfg& cfg, const mrt::TraceVariant& v,
                          const mrt::Workspace* ws, int numRays, int totalLanes, int stackCap, bool blocking) {
    const bool wide = v.nodes != mrt::kNodeCompact2;
    mrt::TraceArgs a{};
    a.nodes = static_cast<const float4*>(wide ? t->wideNodes : t->nodes);
    a.woop = static_cast<const float4*>(t->woop);
    a.triIndex = t->triIndex;
    a.nodeBytes = (uint32_t)(wide ? t->wideBytes : t->nodeBytes);
    a.woopBytes = (uint32_t)t->woopBytes;
    a.numRays = numRays;
    a.numQueues = cfg.num_queues < 0 ? 0 : std::min(cfg.num_queues, std::max(1, numRays));
    // queue_shared percent of the rays past the first round go to the shared queue
    a.sharedRays = a.numQueues > 1 ? (int)((int64_t)numRays * cfg.queue_shared / 100) : 0;
    a.queueBlockLog2 = a.numQueues > 1 && cfg.queue_block > 0 ? __builtin_ctz((unsigned)cfg.queue_block) : 0;
    // the live-lane refill applies to the queue modes only (static rounds hand out one ray per
    // lane per round, to every lane at once): a strided launch reports and uses 0
    a.fetchThreshold = a.numQueues > 0 ? cfg.fetch_threshold : 0;
    a.specSlack = cfg.spec_slack;
    a.staticRounds = cfg.static_rounds;
    a.wideLeafCounts = wide && t->wideLeafCounts;
    a.laneGroupsLog2 = __builtin_ctz((unsigned)cfg.lane_groups);
    a.totalLanes = totalLanes;
    a.stackCap = stackCap;
    a.stackBound = wide ? t->wideStackBound : stackCap - 1;
    a.tailLanes = cfg.tail_lanes;
    a.xccMask = cfg.queue_xcc_mask;
    a.dealBlockLog2 = v.oneshot ? cfg.deal_block : 0;
    a.raySort = cfg.ray_sort;
    a.queues = ws->queues;
    a.spill = ws->spill;
    // The blocking call counts this launch's overflows in a slot of its own; the
    // asynchronous one adds to the sticky counter (mrt_tracer_stack_overflows).
    a.status = blocking ? ws->status + mrt::kTimedSlot : ws->status;
    return a;
}

// Enqueues the launch on s: inside the blocking call's event pair (evStart .. evStop) when
// `blocking`, and inside the autotuner's (tuneStart, tuneStop) when it times this launch.
int enqueue_trace(mrt_tracer* t, const mrt::TraceVariant& v, const mrt::TraceArgs& a, int blocks, int dynLds,
                  mrt::Workspace* ws, hipStream_t s, bool blocking, hipEvent_t tuneStart, hipEvent_t tuneStop) {
    // Queue heads restart at zero for every launch; strided mode has none.
    if (a.numQueues > 0)
        MRT_HIP(hipMemsetAsync(ws->queues, 0, mrt::kQueueLines * mrt::kQueueStrideWords * sizeof(unsigned), s));
    if (blocking) MRT_HIP(hipMemsetAsync(ws->status + mrt::kTimedSlot, 0, sizeof(int), s));
    if (blocking) MRT_HIP(hipEventRecord(t->evStart, s));
    if (tuneStart) MRT_HIP(hipEventRecord(tuneStart, s));
    MRT_HIP(mrt::launch_trace(v, a, blocks, s, dynLds));
#ifdef MRT_DONE_EVENT
    MRT_HIP(hipEventRecord(ws->done, s));
#endif
    ws->launched = true;
    if (tuneStop) MRT_HIP(hipEventRecord(tuneStop, s));
    if (blocking) MRT_HIP(hipEventRecord(t->evStop, s));
    return MRT_OK;
}

// The blocking call: waits for the launch and reports it (the autotune fields are the caller's).
int fill_info(mrt_tracer* t, const mrt::TraceVariant& v, const mrt::TraceArgs& a, const mrt::Workspace* ws,
              mrt_trace_info* info) {
    info->stack_capacity = a.stackCap;
    MRT_HIP(hipEventSynchronize(t->evStop));
    MRT_HIP(hipEventElapsedTime(&info->kernel_ms, t->evStart, t->evStop));
    info->grid_waves = a.totalLanes / 64;
    info->block_threads = mrt::kBlockThreads;
    info->lds_stack_entries = v.ldsStack;
    info->wide = v.nodes != mrt::kNodeCompact2 ? 4 : 2;
    info->node_bytes = v.nodes == mrt::kNodeWide4 ? 128 : 64;
    info->num_queues = a.numQueues;
    info->fetch_threshold = a.fetchThreshold;
    int overflow = 0;
    MRT_HIP(hipMemcpy(&overflow, ws->status + mrt::kTimedSlot, sizeof(int), hipMemcpyDeviceToHost));
    info->stack_overflows = overflow;
    if (overflow)
        return fail(MRT_ERR_STACK_OVERFLOW,
                    std::to_string(overflow) + " stack pushes past the " + std::to_string(a.stackCap) +
                        "-entry traversal stack (stack_capacity): those rays' results are incomplete (BVH "
                        "deeper than the reference's STACK_SIZE 64 allows in the binary order)");
    return MRT_OK;
}

int trace_impl(mrt_tracer* t, const void* rays, void* results, int32_t numRays, uint32_t flags, int32_t* stats,
               void* stream, mrt_trace_info* info) {
    if (int rc = check_call(t, numRays, flags)) return rc;
    std::lock_guard<std::mutex> lock(t->mu);
    if (info) std::memset(info, 0, sizeof(*info));
    if (numRays == 0) return MRT_OK;   // reference CudaTracer.cc:123-125: no rays => 0 ms
    if (int rc = check_batch(t, rays, results, numRays, flags, stats)) return rc;

    DeviceGuard guard(t->device);
    mrt::TraceVariant v = variant_for(t, flags);   // its key (the tracer's tail setting) keys the tuning
    mrt_launch_cfg cfg = mrt::effective_cfg(t->cfg, t->numCUs, t->nodeBytes + t->woopBytes, numRays);
    // autotuning: the schedule candidate this launch uses, and the slot and events of its timing
    mrt::TuneState* tune = t->tunes.lookup(t->cfg, cfg, flags, numRays, variant_key(v), stream);
    int cand = -1, slot = -1;
    hipEvent_t tuneStart = nullptr, tuneStop = nullptr;
    if (tune) {
        tune_collect(tune);
        cand = tune->next_launch(&slot);
        if (slot >= 0)
            if (int rc = tune_events(tune, slot, &tuneStart, &tuneStop)) return rc;
        cfg = mrt::tune_candidate(t->numXccs, cfg, cand, tune);
    }
    v.tail = with_tail(t, v, cfg);   // a tuned candidate may run without the tail
    const int stackCap = v.nodes != mrt::kNodeCompact2 ? t->wideStackCap : mrt::kStackCapacity;
    // cfg.oneshot: the one-shot sibling on the grid planned for it; where the variant has none, the batch
    // fits the resident grid or the slab cap asks for more than one ray per lane, today's kernel and plan
    v.oneshot = cfg.oneshot == 1 && cfg.backfill == 1 && mrt::trace_has_oneshot(v);
    mrt::LaunchPlan plan = launch_plan(t, cfg, v, numRays, stackCap);
    if (v.oneshot && !plan.oneshot) {
        v.oneshot = false;
        plan = launch_plan(t, cfg, v, numRays, stackCap);
    }
    const int blocks = plan.blocks;
    const int totalLanes = blocks * mrt::kBlockThreads;
    mrt::Workspace* ws = nullptr;
    if (int rc = workspace_for(t, stream, totalLanes, v.ldsStack, stackCap, &ws)) return rc;

    mrt::TraceArgs a = trace_args(t, cfg, v, ws, numRays, totalLanes, stackCap, info != nullptr);
    a.rays = static_cast<const float4*>(rays);
    a.results = static_cast<int2*>(results);
    a.stats = reinterpret_cast<int4*>(stats);
    if (int rc = enqueue_trace(t, v, a, blocks, plan.dynLds, ws, static_cast<hipStream_t>(stream), info != nullptr,
                               tuneStart, tuneStop))
        return rc;
    if (slot >= 0) tune->slot_started(slot, cand);
    if (!info) return MRT_OK;
    info->autotune_candidate = tune ? tune->info_code(cand) : -1;
    info->autotune_locked = tune && tune->locked >= 0 ? 1 : 0;
    info->backfill = plan.backfill;
    info->oneshot = plan.oneshot;
    info->deal_block = plan.oneshot ? plan.dealBlockLog2 : 0;
    info->blocks_per_cu = plan.blocksPerCU;
    info->dyn_lds_bytes = plan.dynLds;
    return fill_info(t, v, a, ws, info);
}

// ---- refit (mrt_tracer_refit): the plan and the launches ---------------------------

// Builds the refit plan of the bound tree (the handle's mutex held). Synchronous: the
// Compact2 nodes come to the host once for their child refs (topology only: a refit in
// flight changes boxes, never words 12-15).
int build_plan(mrt_tracer* t) {
    if (t->planBuilt) return MRT_OK;
    const int64_t numNodes = t->nodeBytes / 64;
    std::vector<int32_t> host((size_t)(t->nodeBytes / 4));
    MRT_HIP(hipMemcpy(host.data(), t->nodes, (size_t)t->nodeBytes, hipMemcpyDeviceToHost));
    mrt::RefitLevels lv;
    if (const char* why = mrt::refit_levels(host.data(), numNodes, &lv))
        return fail(MRT_ERR_INVALID_ARG, std::string("refit: the bound nodes are not a tree: ") + why);
    std::vector<int32_t> offsets(lv.offsets.begin(), lv.offsets.end());   // < 2^26 nodes
    drop_plan(t);
    MRT_HIP(hipMalloc(&t->planOrder, lv.order.size() * 4));
    MRT_HIP(hipMemcpy(t->planOrder, lv.order.data(), lv.order.size() * 4, hipMemcpyHostToDevice));
    MRT_HIP(hipMalloc(&t->planOffsets, offsets.size() * 4));
    MRT_HIP(hipMemcpy(t->planOffsets, offsets.data(), offsets.size() * 4, hipMemcpyHostToDevice));
    MRT_HIP(hipMalloc(&t->planValid, (size_t)numNodes * 2));
    MRT_HIP(hipMalloc(&t->planSkipped, sizeof(unsigned long long)));
    MRT_HIP(hipMemset(t->planSkipped, 0, sizeof(unsigned long long)));
    t->planBytes = (int64_t)lv.order.size() * 4 + (int64_t)offsets.size() * 4 + numNodes * 2 + 8;
    if (t->wideNodes && t->wideFormat == mrt::kNodeWide4 && (int64_t)t->wideSrc.size() == t->wideBytes / 128 * 4) {
        MRT_HIP(hipMalloc(&t->planWideSrc, t->wideSrc.size() * 4));
        MRT_HIP(hipMemcpy(t->planWideSrc, t->wideSrc.data(), t->wideSrc.size() * 4, hipMemcpyHostToDevice));
        t->planBytes += (int64_t)t->wideSrc.size() * 4;
    }
    t->planLevels = lv.offsets;
    t->planBuilt = true;
    return MRT_OK;
}

// The Woop rows and boxes of the Compact2 buffers in `a`, bound or not: the leaves, one launch
// per level above kRefitTailNodes nodes, one workgroup for all smaller levels. levels: the
// plan's offsets on the host; order / offsets: the plan on the device.
int enqueue_refit(const mrt::RefitArgs& a, const std::vector<int64_t>& levelOffsets, const int32_t* order,
                  const int32_t* offsets, hipStream_t s, int* launches) {
    MRT_HIP(mrt::launch_refit_leaves(a, s));
    ++*launches;
    const int levels = (int)levelOffsets.size() - 1;
    for (int l = 1; l < levels; l++) {
        const int begin = (int)levelOffsets[(size_t)l], count = (int)(levelOffsets[(size_t)l + 1] - begin);
        if (count > mrt::kRefitTailNodes) {
            MRT_HIP(mrt::launch_refit_level(a, order, begin, count, s));
            ++*launches;
            continue;
        }
        // level sizes never grow with the height: this one and all above it fit one workgroup
        MRT_HIP(mrt::launch_refit_tail(a, order, offsets, l, levels, s));
        ++*launches;
        break;
    }
    return MRT_OK;
}

int refit_impl(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
               int64_t numTriangles, void* stream) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    if (numVertices < 0 || numTriangles < 0 || (numVertices && !vertices) || (numTriangles && !triangles))
        return fail(MRT_ERR_INVALID_ARG, "refit: bad vertex / triangle arrays");
    std::lock_guard<std::mutex> lock(t->mu);
    if (!t->bound) return fail(MRT_ERR_NOT_BOUND, "refit before bind (no BVH)");
    DeviceGuard guard(t->device);
    if (int rc = build_plan(t)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    mrt::RefitArgs a{};
    a.nodes = static_cast<uint32_t*>(const_cast<void*>(t->nodes));   // refit writes the bound buffers (mrt.h)
    a.numNodes = (int)(t->nodeBytes / 64);
    a.woop = static_cast<uint32_t*>(const_cast<void*>(t->woop));
    a.woopSlots = (int)(t->woopBytes / 16);
    a.triIndex = t->triIndex;
    a.vertices = vertices;
    a.numVertices = numVertices;
    a.triangles = triangles;
    a.numTriangles = numTriangles;
    a.valid = t->planValid;
    a.skipped = t->planSkipped;

    int launches = 0;
    t->refitLaunched = true;
    if (int rc = enqueue_refit(a, t->planLevels, t->planOrder, t->planOffsets, s, &launches)) return rc;
    if (t->planWideSrc && t->wideNodes && t->wideFormat == mrt::kNodeWide4) {
        MRT_HIP(mrt::launch_refit_wide(a, t->planWideSrc, static_cast<uint32_t*>(t->wideNodes), (int)(t->wideBytes / 128), s));
        launches++;
    }
    t->refitLaunches = launches;
    if (t->wideNodes && t->wideFormat == mrt::kNodeWide4Q) {
        // The quantized form has no in-place update: derive it again from the refitted
        // nodes through the bind-time host path (synchronous and slow; mrt.h).
        MRT_HIP(hipStreamSynchronize(s));
        t->wideBuiltFor = -1;
        if (int rc = refresh_wide(t)) return rc;
        // the exact form as a fallback would need a new source map on the device
        if (t->wideFormat == mrt::kNodeWide4) {
            t->planBuilt = false;
            return build_plan(t);
        }
    }
    return MRT_OK;
}

// ---- device build (mrt_tracer_build): scratch, phases, the plan, the bind -----------

int check_build_count(int64_t numTriangles) {
    if (numTriangles < 1) return fail(MRT_ERR_INVALID_ARG, "build: numTriangles < 1");
    if (numTriangles > mrt::lbvh::kMaxTriangles)
        return fail(MRT_ERR_TOO_LARGE, "build: more than 67108863 triangles (2^28 Woop slots, the refit's limit)");
    return MRT_OK;
}

// The stream-ordered scratch and the phase events of one build, returned on every way out.
struct BuildTemps {
    hipStream_t s = nullptr;
    void* scratch = nullptr;
    hipEvent_t ev[5] = {};
    ~BuildTemps() {
        if (scratch) (void)hipFreeAsync(scratch, s);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int build_impl(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
               int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity, void* woop,
               int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity, int64_t* nodeBytes,
               int64_t* woopBytes, int64_t* triIndexBytes, void* stream) {
    int maxLeaf = params ? params->max_leaf_size : 0;
    if (maxLeaf < 0 || maxLeaf > mrt::lbvh::kMaxLeafLimit) return fail(MRT_ERR_INVALID_ARG, "build: max_leaf_size outside 0..8");
    if (maxLeaf == 0) maxLeaf = MRT_LBVH_DEFAULT_MAX_LEAF;
    if (numVertices < 0) return fail(MRT_ERR_INVALID_ARG, "build: numVertices < 0");
    if (int rc = check_build_count(numTriangles)) return rc;
    if (!t || (numVertices && !vertices) || !triangles || !nodes || !woop || !triIndex || !nodeBytes || !woopBytes ||
        !triIndexBytes)
        return fail(MRT_ERR_INVALID_ARG, "build: null argument");
    const int n = (int)numTriangles;
    const int64_t maxRecords = mrt::lbvh::max_records(n), maxSlots = mrt::lbvh::max_slots(n);
    if (nodeCapacity < maxRecords * 64 || woopCapacity < maxSlots * 16 || triIndexCapacity < maxSlots * 4)
        return fail(MRT_ERR_TOO_LARGE, "build: an output capacity is below mrt_lbvh_sizes");

    std::lock_guard<std::mutex> lock(t->mu);
    DeviceGuard guard(t->device);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = static_cast<hipStream_t>(stream);

    // Scratch: the topology's (lbvh_kernel.hip), then the refit's valid flags, skipped
    // counter and level plan, each on a 256-byte boundary.
    size_t topoBytes = 0, primBytes = 0;
    MRT_HIP(mrt::lbvh_scratch_bytes(n, &topoBytes, &primBytes));
    auto aligned = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t validAt = aligned(topoBytes), skippedAt = validAt + aligned((size_t)maxRecords * 2),
                 orderAt = skippedAt + 256, offsetsAt = orderAt + aligned((size_t)maxRecords * 4),
                 total = offsetsAt + aligned(((size_t)maxRecords + 1) * 4);
    BuildTemps tmp;
    tmp.s = s;
    MRT_HIP(hipMallocAsync(&tmp.scratch, total, s));
    for (hipEvent_t& e : tmp.ev) MRT_HIP(hipEventCreate(&e));
    char* base = static_cast<char*>(tmp.scratch);
    auto* skippedDev = reinterpret_cast<unsigned long long*>(base + skippedAt);
    auto* orderDev = reinterpret_cast<int32_t*>(base + orderAt);
    auto* offsetsDev = reinterpret_cast<int32_t*>(base + offsetsAt);

    mrt::LbvhBuild b{};
    b.vertices = vertices;
    b.numVertices = numVertices;
    b.triangles = triangles;
    b.numTriangles = n;
    b.maxLeaf = maxLeaf;
    b.nodes = static_cast<uint32_t*>(nodes);
    b.woop = static_cast<uint32_t*>(woop);
    b.triIndex = triIndex;
    mrt::lbvh_carve(b, tmp.scratch, primBytes);

    // Phase 1: keys and order. Phase 2: hierarchy and emission.
    const bool single = n <= maxLeaf;
    MRT_HIP(hipEventRecord(tmp.ev[0], s));
    MRT_HIP(mrt::launch_lbvh_sort(b, s));
    MRT_HIP(hipEventRecord(tmp.ev[1], s));
    MRT_HIP(single ? mrt::launch_lbvh_emit_single(b, s) : mrt::launch_lbvh_emit(b, s));
    MRT_HIP(hipEventRecord(tmp.ev[2], s));
    int32_t records = 1, leaves = 2;
    if (!single) {
        MRT_HIP(hipMemcpyAsync(&records, b.keptRank + (n - 1), 4, hipMemcpyDeviceToHost, s));
        MRT_HIP(hipMemcpyAsync(&leaves, b.leafRank + n, 4, hipMemcpyDeviceToHost, s));
    }
    MRT_HIP(hipStreamSynchronize(s));
    if (records < 1 || records > maxRecords || leaves < 1 || leaves > n + 1)
        return fail(MRT_ERR_HIP, "build: the emitted counts are inconsistent");
    const int64_t slots = 3 * (int64_t)n + leaves;

    // The level plan of the emitted topology, on the host (the call is synchronous for it).
    const auto tPlan = std::chrono::steady_clock::now();
    std::vector<int32_t> host((size_t)records * 16);
    MRT_HIP(hipMemcpyAsync(host.data(), nodes, host.size() * 4, hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));
    mrt::RefitLevels lv;
    if (const char* why = mrt::refit_levels(host.data(), records, &lv))
        return fail(MRT_ERR_HIP, std::string("build: the emitted nodes are not a tree: ") + why);
    const std::vector<int32_t> offsets(lv.offsets.begin(), lv.offsets.end());
    MRT_HIP(hipMemcpyAsync(orderDev, lv.order.data(), lv.order.size() * 4, hipMemcpyHostToDevice, s));
    MRT_HIP(hipMemcpyAsync(offsetsDev, offsets.data(), offsets.size() * 4, hipMemcpyHostToDevice, s));
    MRT_HIP(hipMemsetAsync(skippedDev, 0, sizeof(unsigned long long), s));
    MRT_HIP(hipStreamSynchronize(s));   // the uploads read lv and offsets
    const double planMs = ms_since(tPlan);

    // Phase 3: Woop rows and boxes, by the refit's launches on the buffers not yet bound.
    mrt::RefitArgs a{};
    a.nodes = b.nodes;
    a.numNodes = records;
    a.woop = b.woop;
    a.woopSlots = (int)slots;
    a.triIndex = triIndex;
    a.vertices = vertices;
    a.numVertices = numVertices;
    a.triangles = triangles;
    a.numTriangles = n;
    a.valid = reinterpret_cast<uint8_t*>(base + validAt);
    a.skipped = skippedDev;
    int launches = 0;
    MRT_HIP(hipEventRecord(tmp.ev[3], s));
    if (int rc = enqueue_refit(a, lv.offsets, orderDev, offsetsDev, s, &launches)) return rc;
    if (single) MRT_HIP(mrt::launch_lbvh_empty_leaf_box(b.nodes, s));
    MRT_HIP(hipEventRecord(tmp.ev[4], s));
    unsigned long long skipped = 0;
    MRT_HIP(hipMemcpyAsync(&skipped, skippedDev, sizeof(skipped), hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));

    mrt_build_info info{};
    MRT_HIP(hipEventElapsedTime(&info.sort_ms, tmp.ev[0], tmp.ev[1]));
    MRT_HIP(hipEventElapsedTime(&info.emit_ms, tmp.ev[1], tmp.ev[2]));
    MRT_HIP(hipEventElapsedTime(&info.fit_ms, tmp.ev[3], tmp.ev[4]));

    if (int rc = bind_locked(t, nodes, (int64_t)records * 64, woop, slots * 16, triIndex, slots * 4)) return rc;
    info.plan_ms = planMs;
    info.bind_ms = t->bindMs;
    info.levels = lv.levels();
    info.records = records;
    info.leaves = leaves;
    info.slots = slots;
    info.scratch_bytes = (int64_t)total;
    info.skipped_refs = (int64_t)skipped;
    info.max_leaf_size = maxLeaf;
    info.wall_ms = ms_since(t0);
    t->lastBuild = info;
    *nodeBytes = (int64_t)records * 64;
    *woopBytes = slots * 16;
    *triIndexBytes = slots * 4;
    return MRT_OK;
}

}  // namespace

extern "C" {

int mrt_version(void) { return 100; }

const char* mrt_error_string(int err) {
    switch (err) {
        case MRT_OK: return "ok";
        case MRT_ERR_INVALID_ARG: return "invalid argument";
        case MRT_ERR_NOT_BOUND: return "no BVH bound";
        case MRT_ERR_HIP: return "HIP runtime error";
        case MRT_ERR_NO_DEVICE: return "no HIP device";
        case MRT_ERR_TOO_LARGE: return "buffer or batch too large";
        case MRT_ERR_STACK_OVERFLOW: return "traversal stack overflow";
        default: return "unknown error";
    }
}

const char* mrt_last_error_detail(void) { return mrt::api_last_error(); }

int mrt_selftest_exact_rcp(uint64_t* mismatches) {
    if (!mismatches) return fail(MRT_ERR_INVALID_ARG, "null argument");
    unsigned long long* d = nullptr;
    MRT_HIP(hipMalloc(&d, sizeof(*d)));
    hipError_t e = hipMemset(d, 0, sizeof(*d));
    if (e == hipSuccess) e = mrt::selftest_exact_rcp(d, nullptr);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hipFail(e, "selftest_exact_rcp");
    *mismatches = h;
    return MRT_OK;
}

int mrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mrt_tracer_create(int device, mrt_tracer** out) {
    if (!out) return fail(MRT_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MRT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(MRT_ERR_INVALID_ARG, "device index out of range");
    int cus = 0, xccs = 0;
    MRT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    // XCDs of this device (partition): the HIP attribute, else 32 CUs per MI355X XCD
    if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, device) != hipSuccess || xccs <= 0)
        xccs = std::max(1, cus / 32);
    mrt_tracer* t = new mrt_tracer();
    t->device = device;
    t->numCUs = cus;
    t->numXccs = std::max(1, std::min(xccs, mrt::kMaxQueues));
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && lds > 0)
        t->ldsPerCU = lds;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0)
        t->ldsPerBlock = lds;
    t->cfg = default_cfg();
    *out = t;
    return MRT_OK;
}

int mrt_tracer_destroy(mrt_tracer* t) {
    if (!t) return MRT_OK;
    {
        DeviceGuard guard(t->device);
        drop_plan(t);
        if (t->wideNodes) (void)hipFree(t->wideNodes);
        (void)wait_all_workspaces(t);   // event waits: the streams may already be destroyed
        for (mrt::Workspace* w : t->workspaces) {
            if (w->done) (void)hipEventDestroy(w->done);
            if (w->queues) (void)hipFree(w->queues);
            if (w->status) (void)hipFree(w->status);
            if (w->spill) (void)hipFree(w->spill);
            delete w;
        }
        if (t->evStart) (void)hipEventDestroy(t->evStart);
        if (t->evStop) (void)hipEventDestroy(t->evStop);
        tune_reset(t);
    }
    delete t;
    return MRT_OK;
}

int mrt_tracer_bind(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                    const int32_t* triIndex, int64_t triIndexBytes) {
    if (!t || !nodes || !woop || !triIndex) return fail(MRT_ERR_INVALID_ARG, "null BVH buffer");
    if (nodeBytes < 64 || woopBytes < 16 || triIndexBytes < 4 || (nodeBytes % 64) || (woopBytes % 16) ||
        (triIndexBytes % 4))
        return fail(MRT_ERR_INVALID_ARG, "BVH buffer sizes are not Compact2-shaped");
    if (nodeBytes > mrt::kMaxBufferBytes || woopBytes > mrt::kMaxBufferBytes)
        return fail(MRT_ERR_TOO_LARGE, "Compact2 buffer above the 32-bit buffer-offset range");
    if (triIndexBytes / 4 != woopBytes / 16) return fail(MRT_ERR_INVALID_ARG, "triIndex must hold one int per woop float4");
    std::lock_guard<std::mutex> lock(t->mu);
    return bind_locked(t, nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes);
}

int mrt_tracer_unbind(mrt_tracer* t) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    std::lock_guard<std::mutex> lock(t->mu);
    t->bound = false;
    t->nodes = t->woop = nullptr;
    t->triIndex = nullptr;
    DeviceGuard guard(t->device);
    drop_plan(t);
    return refresh_wide(t);
}

int mrt_tracer_set_config(mrt_tracer* t, const mrt_launch_cfg* cfg) {
    if (!t || !cfg) return fail(MRT_ERR_INVALID_ARG, "null argument");
    mrt_launch_cfg c = *cfg;
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
    if (!valid_cfg(c)) return fail(MRT_ERR_INVALID_ARG, "launch config out of range");
    std::lock_guard<std::mutex> lock(t->mu);
    t->cfg = c;
    DeviceGuard guard(t->device);
    tune_reset(t);
    drop_plan(t);
    const auto t0 = std::chrono::steady_clock::now();
    const int built = t->wideBuiltFor;
    const int rc = refresh_wide(t);
    if (t->wideBuiltFor != built)
        t->bindMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int mrt_tracer_get_config(const mrt_tracer* t, mrt_launch_cfg* cfg) {
    if (!t || !cfg) return fail(MRT_ERR_INVALID_ARG, "null argument");
    *cfg = t->cfg;
    return MRT_OK;
}

int mrt_tracer_bind_info(const mrt_tracer* t, mrt_bind_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    info->bind_ms = t->bindMs;
    info->wide_bytes = t->wideNodes ? t->wideBytes : 0;
    info->wide_format = t->wideNodes ? t->wideFormat : mrt::kNodeCompact2;
    info->stack_capacity = t->wideNodes ? t->wideStackCap : mrt::kStackCapacity;
    info->stack_bound = t->wideNodes ? t->wideStackBound : mrt::kStackCapacity - 1;
    return MRT_OK;
}

int mrt_tracer_tune_export(const mrt_tracer* t, mrt_tuned_schedule* out, int32_t capacity, int32_t* count) {
    if (!t || !count || (capacity > 0 && !out)) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<mrt_tracer*>(t)->mu);
    *count = t->tunes.export_schedules(out, capacity);
    return MRT_OK;
}

int mrt_tracer_tune_import(mrt_tracer* t, const mrt_tuned_schedule* in, int32_t count) {
    if (!t || (count > 0 && !in) || count < 0) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    const int rc = t->tunes.import_schedules(in, count);
    if (rc == MRT_ERR_INVALID_ARG) return fail(rc, "tuned schedule from another library version or out of range");
    if (rc == MRT_ERR_TOO_LARGE) return fail(rc, "more tuned batch sizes than kMaxTuned");
    return rc;
}

int mrt_tracer_trace(mrt_tracer* t, const void* rays, void* results, int32_t numRays, uint32_t flags,
                     int32_t* stats, void* stream) {
    return trace_impl(t, rays, results, numRays, flags, stats, stream, nullptr);
}

int mrt_tracer_trace_timed(mrt_tracer* t, const void* rays, void* results, int32_t numRays, uint32_t flags,
                           int32_t* stats, void* stream, mrt_trace_info* info) {
    mrt_trace_info local;
    return trace_impl(t, rays, results, numRays, flags, stats, stream, info ? info : &local);
}

int mrt_tracer_stack_overflows(mrt_tracer* t, int64_t* count, int32_t reset) {
    if (!t || !count) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    DeviceGuard guard(t->device);
    int64_t total = 0;
    for (mrt::Workspace* w : t->workspaces) {
        int n = 0;
        if (int rc = workspace_wait(w)) return rc;
        MRT_HIP(hipMemcpy(&n, w->status, sizeof(int), hipMemcpyDeviceToHost));
        total += n;
        if (reset) MRT_HIP(hipMemset(w->status, 0, sizeof(int)));
    }
    *count = total;
    return MRT_OK;
}

int mrt_tracer_refit(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                     int64_t numTriangles, void* stream) {
    return refit_impl(t, vertices, numVertices, triangles, numTriangles, stream);
}

int mrt_tracer_refit_info(mrt_tracer* t, mrt_refit_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    std::memset(info, 0, sizeof(*info));
    if (!t->planBuilt) return MRT_OK;
    DeviceGuard guard(t->device);
    if (t->refitLaunched) MRT_HIP(hipDeviceSynchronize());
    t->refitLaunched = false;
    unsigned long long skipped = 0;
    MRT_HIP(hipMemcpy(&skipped, t->planSkipped, sizeof(skipped), hipMemcpyDeviceToHost));
    MRT_HIP(hipMemset(t->planSkipped, 0, sizeof(skipped)));
    info->levels = (int32_t)t->planLevels.size() - 1;
    info->launches = t->refitLaunches;
    info->plan_bytes = t->planBytes;
    info->skipped_refs = (int64_t)skipped;
    return MRT_OK;
}

int mrt_lbvh_sizes(int64_t numTriangles, int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes) {
    if (!nodeBytes || !woopBytes || !triIndexBytes) return fail(MRT_ERR_INVALID_ARG, "lbvh_sizes: null argument");
    if (int rc = check_build_count(numTriangles)) return rc;
    *nodeBytes = mrt::lbvh::max_records(numTriangles) * 64;
    *woopBytes = mrt::lbvh::max_slots(numTriangles) * 16;
    *triIndexBytes = mrt::lbvh::max_slots(numTriangles) * 4;
    return MRT_OK;
}

int mrt_tracer_build(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                     int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity,
                     void* woop, int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity,
                     int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes, void* stream) {
    return build_impl(t, vertices, numVertices, triangles, numTriangles, params, nodes, nodeCapacity, woop, woopCapacity,
                      triIndex, triIndexCapacity, nodeBytes, woopBytes, triIndexBytes, stream);
}

int mrt_tracer_build_info(mrt_tracer* t, mrt_build_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    *info = t->lastBuild;
    return MRT_OK;
}

int mrt_tracer_copy_wide_nodes(mrt_tracer* t, void* out, int64_t capacity, int64_t* bytes) {
    if (!t || !bytes) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    *bytes = t->wideNodes ? t->wideBytes : 0;
    if (!out || *bytes == 0) return MRT_OK;
    if (capacity < *bytes) return fail(MRT_ERR_TOO_LARGE, "copy_wide_nodes: output buffer too small");
    DeviceGuard guard(t->device);
    MRT_HIP(hipDeviceSynchronize());   // refits in flight on any stream write the array
    t->refitLaunched = false;
    MRT_HIP(hipMemcpy(out, t->wideNodes, (size_t)*bytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}

int mrt_refit_plan(const void* nodes, int64_t nodeBytes, int32_t* order, int64_t* levelOffsets, int32_t levelCapacity,
                   int32_t* numLevels, int32_t* wideSrc, int64_t wideSrcCapacity, int64_t* numWideSrc) {
    if (!nodes || nodeBytes <= 0 || nodeBytes % 64 != 0 || !numLevels || levelCapacity < 0 || wideSrcCapacity < 0)
        return fail(MRT_ERR_INVALID_ARG, "refit_plan: bad arguments");
    const auto* n = static_cast<const int32_t*>(nodes);
    mrt::RefitLevels lv;
    if (const char* why = mrt::refit_levels(n, nodeBytes / 64, &lv))
        return fail(MRT_ERR_INVALID_ARG, std::string("refit_plan: ") + why);
    *numLevels = lv.levels();
    if (order) std::memcpy(order, lv.order.data(), lv.order.size() * 4);
    if (levelOffsets) {
        if (levelCapacity < (int32_t)lv.offsets.size()) return fail(MRT_ERR_TOO_LARGE, "refit_plan: levelOffsets too small");
        std::memcpy(levelOffsets, lv.offsets.data(), lv.offsets.size() * 8);
    }
    if (numWideSrc) {
        std::vector<int32_t> src;
        (void)mrt::build_wide4(n, nodeBytes / 64, nullptr, 0, &src);
        *numWideSrc = (int64_t)src.size();
        if (wideSrc) {
            if (wideSrcCapacity < *numWideSrc) return fail(MRT_ERR_TOO_LARGE, "refit_plan: wideSrc too small");
            std::memcpy(wideSrc, src.data(), src.size() * 4);
        }
    }
    return MRT_OK;
}

int mrt_derive_wide_nodes(const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes, int32_t form,
                          void* out, int64_t outCapacity, int64_t* outBytes) {
    if (!nodes || !outBytes || nodeBytes <= 0 || nodeBytes % 64 != 0 || (form != 1 && form != 2) ||
        (woop && (woopBytes <= 0 || woopBytes % 16 != 0)))
        return fail(MRT_ERR_INVALID_ARG, "derive_wide_nodes: bad arguments");
    // the first word of every Woop slot, when the leaf refs can carry counts
    const int64_t slots = woop ? woopBytes / 16 : 0;
    std::vector<int32_t> woopX;
    if (woop && mrt::leaf_counts_fit(slots)) {
        woopX.resize((size_t)slots);
        for (int64_t i = 0; i < slots; i++) woopX[(size_t)i] = static_cast<const int32_t*>(woop)[4 * i];
    }
    const int32_t* wx = woopX.empty() ? nullptr : woopX.data();
    std::vector<uint32_t> wide;
    const auto* n = static_cast<const int32_t*>(nodes);
    if (form == 2) {
        if (!mrt::build_wide4q(n, nodeBytes / 64, &wide, wx, slots))
            return fail(MRT_ERR_INVALID_ARG, "a box has no finite quantization");
    } else {
        wide = mrt::build_wide4(n, nodeBytes / 64, wx, slots);
    }
    *outBytes = (int64_t)wide.size() * 4;
    if (out) {
        if (outCapacity < *outBytes) return fail(MRT_ERR_TOO_LARGE, "derive_wide_nodes: output buffer too small");
        std::memcpy(out, wide.data(), (size_t)*outBytes);
    }
    return MRT_OK;
}

}  // extern "C"
