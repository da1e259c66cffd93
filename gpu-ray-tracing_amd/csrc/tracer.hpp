// tracer.hpp — the tracer handle behind include/mrt.h and the functions of one C-ABI file that
// another one calls. The handle's sub-objects own their device memory and events; each file
// works on its own: the handle's lifecycle, configuration, workspace pool, tune events and the
// trace path (mrt_api.cpp), bind and the 4-wide derivation (bind_api.cpp), refit (refit_api.cpp),
// the device build (build_api.cpp), the plan and the 4-wide array derived on the device
// (derive_api.cpp), the treelet restructuring (optimize_api.cpp).
#pragma once
#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "api_common.hpp"
#include "refit_kernel.hpp"
#include "tune.hpp"
#include "wide_kernel.hpp"

namespace mrt {

// 4-wide nodes derived from the bound Compact2 tree (cfg.wide; wide_bvh.cpp), owned by the
// tracer and rebuilt when the BVH or the setting changes (refresh_wide).
struct WideArray {
    DeviceBuf<uint32_t> nodes;
    int64_t bytes = 0;
    int builtFor = -1;             // the cfg.wide value the current array was built for
    int format = kNodeCompact2;    // the form `nodes` holds (kNodeWide4 / kNodeWide4Q)
    bool leafCounts = false;       // its leaf refs carry triangle counts
    // Stack entries (sentinel included) the wide traversal gets: the wide tree's
    // worst case (wide_stack_bound) + 1, at least the reference's 64. A wide node
    // pushes up to three children where the binary step pushes one, so a tree that
    // fits the reference's stack in binary order could otherwise overflow in wide
    // order; sized this way no ray of the bound tree can overflow it.
    int stackCap = kStackCapacity;
    int stackBound = kStackCapacity - 1;   // wide_stack_bound of the derived tree (the tail's headroom)
    // Exact form only: per wide child the Compact2 slot (binary node * 2 + side) its box was
    // copied from, -1 = absent — from the collapse that produced `nodes` (a refit copies the
    // refitted boxes along it; collapsing refitted nodes again would choose other children).
    std::vector<int32_t> src;
    // The same map where the array was derived on the device (derive_api.cpp): it lives only
    // there, `src` stays empty, and a refit reads it in place of the plan's copy.
    DeviceBuf<int32_t> srcDev;
};

// Largest wide-traversal stack a tracer sizes its spill slab for (entries per lane).
constexpr int kMaxWideStack = 1024;

// The refit plan (mrt_tracer_refit), built on the first refit after a bind or set_config
// and dropped by bind, unbind and set_config (drop_plan): the nodes by height level, the wide
// source map and the refit's scratch, on the device.
struct RefitPlan {
    bool built = false;
    DeviceBuf<int32_t> order;      // numNodes node indices, level by level
    DeviceBuf<int32_t> offsets;    // levels + 1 offsets into order
    DeviceBuf<int32_t> wideSrc;    // WideArray::src on the device (null: no exact wide array, or WideArray::srcDev)
    DeviceBuf<uint8_t> valid;      // 2 per node, rewritten by every refit
    DeviceBuf<unsigned long long> skipped;   // out-of-range references skipped since the last refit_info
    std::vector<int64_t> levels;   // the level offsets on the host
    int64_t bytes = 0;
    int launches = 0;              // kernel launches of the last refit
    bool launched = false;         // a refit may still be running (wait_refit)
};

// Launch scratch of one stream (workspace_for).
struct Workspace {
    void* stream = nullptr;       // the hipStream_t this scratch was last used on
    DeviceBuf<unsigned> queues;   // kQueueLines * kQueueStrideWords words
    DeviceBuf<int> status;        // [0] = stack overflows of asynchronous launches since the last reset
                                  // (sticky); [kTimedSlot] = the current blocking launch's own count
    DeviceBuf<int> spill;
    size_t spillInts = 0;
    // -DMRT_DONE_EVENT: recorded after every launch that uses this scratch, so waiting
    // for it never touches the stream (see workspace_wait)
    Event done;
    bool launched = false;        // a launch may still be using this scratch
    uint64_t lastUse = 0;         // launch counter value of the last use (LRU reuse)
};

// One derivation on the device (derive_api.cpp): its stream-ordered scratch, the depth levels
// the topology pass found, the phase events and what mrt_tracer_derive_info counts.
struct DeriveRun {
    wide::Derive d{};
    DeriveScratch x{};
    std::vector<int32_t> depth;      // depth level starts into d.byDepth, depthLevels + 1 entries
    std::vector<int32_t> offsets32;  // the height level starts, read back from the device
    int depthLevels = 0;
    int launches = 0, readbacks = 0;
    size_t scratchBytes = 0;
    Event ev[5];                     // topology begin / end, collapse begin, emission begin / end
    StreamScratch scratch;           // last: freed on its stream before the events go
};
enum : int { kDeriveOk = 0, kDeriveMalformed = 1, kDeriveTooDeep = 2 };

// The event pairs of a TuneState's timing slots (created lazily, destroyed in tune_reset).
struct TuneEvents {
    EventPair slot[TuneState::kSlots];
};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace mrt

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

    mrt::WideArray wide;
    double bindMs = 0.0;               // wall time of the last bind / wide derivation (mrt_trace_info)
    mrt::RefitPlan plan;
    mrt_build_info lastBuild{};        // the last successful mrt_tracer_build (mrt_tracer_build_info)
    mrt_derive_info lastDerive{};      // the last device bind / build / plan (mrt_tracer_derive_info)
    mrt_optimize_info lastOptimize{};  // the last successful mrt_tracer_optimize (mrt_tracer_optimize_info)

    // Launch scratch, one set per stream the handle has launched on: the stack
    // spill slab, the queue heads and the overflow counter are written by a
    // running trace, so two traces in flight on different streams must not
    // share them (the handle's mutex only covers enqueueing). A set is complete
    // (queues and status allocated) before it enters the list, and stays where it is.
    std::vector<std::unique_ptr<mrt::Workspace>> workspaces;
    uint64_t useClock = 0;   // launches of this handle (the workspaces' LRU order; guarded by mu)
    mrt::EventPair blocking; // the blocking call's timing pair (created with the first workspace)

    // Occupancy per kernel (index kernel_key(), below 1024), queried once
    // (hipOccupancy* is a host round-trip that would otherwise sit on every launch).
    int occ[1024] = {};
    // Backfilled launches (launch_plan.hpp): per variant and residency cap of 1..kMaxCapBlocks
    // workgroups per CU, the dynamic LDS bytes + 1 that the occupancy query confirmed to give
    // exactly that residency (0: not asked yet, -1: none found, such launches run persistent).
    static constexpr int kMaxCapBlocks = 8;
    int capDyn[1024][kMaxCapBlocks + 1] = {};
    int staticLds[1024] = {};   // per kernel: its static LDS bytes + 1 (0: not asked yet)
    const void* lastKernel = nullptr;   // the kernel function of the most recent launch (mrt_tracer_last_kernel_key)

    // cfg.autotune: per (batch size, variant) the ray-distribution schedule the
    // measured launches chose (tune.cpp), reset on bind/set_config.
    mrt::TuneTable tunes;
};

namespace mrt {

// Those that take the handle are called with its mutex held and its device current.

// mrt_api.cpp: every launch of this handle has completed; the tuned schedules are forgotten.
int wait_all_workspaces(mrt_tracer* t);
void tune_reset(mrt_tracer* t);

// bind_api.cpp: the bind itself, arguments checked (mrt_tracer_bind, mrt_tracer_build), and the
// 4-wide nodes (re)derived when cfg.wide or the bound BVH asks for another array than the one held.
int bind_locked(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                const int32_t* triIndex, int64_t triIndexBytes);
int refresh_wide(mrt_tracer* t);
int check_bind_args(const mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                    const int32_t* triIndex, int64_t triIndexBytes);
void unbind_locked(mrt_tracer* t);

// refit_api.cpp: waits for a refit that may still run (it reads the plan and writes the wide
// array); forgets the plan; the refit's launches on Compact2 buffers, bound or not.
int wait_refit(mrt_tracer* t);
void drop_plan(mrt_tracer* t);
int enqueue_refit(const RefitArgs& a, const std::vector<int64_t>& levelOffsets, const int32_t* order,
                  const int32_t* offsets, hipStream_t s, int* launches);

// derive_api.cpp: the refit plan and the exact 4-wide array derived on the device (wide_kernel.hip).
// derive_begin takes the scratch for `numNodes` records at `nodes`; derive_plan fills p (order,
// offsets, levels, valid, skipped; not wideSrc, not built) and sets *status: kDeriveMalformed
// with *why = refit_levels' reason, kDeriveTooDeep above MRT_DERIVE_MAX_LEVELS depth levels (the
// caller takes the host path). bind_derived is bind_locked for a tree whose plan p was derived
// by r: the bookkeeping, the wide array per cfg.wide, the plan installed (keepTunes: the same
// buffers re-installed by optimize_api.cpp, the tuned schedules stay). All enqueue on s;
// bind_derived returns after the device has finished. derive_report fills t->lastDerive.
int derive_begin(DeriveRun& r, const void* nodes, int64_t numNodes, hipStream_t s);
int derive_plan(DeriveRun& r, RefitPlan* p, hipStream_t s, int* status, const char** why);
int bind_derived(mrt_tracer* t, DeriveRun& r, RefitPlan&& p, const void* nodes, int64_t nodeBytes, const void* woop,
                 int64_t woopBytes, const int32_t* triIndex, int64_t triIndexBytes, hipStream_t s, bool keepTunes = false);
int derive_report(mrt_tracer* t, const DeriveRun& r, bool plan, bool wide, double wallMs);
// The source map a refit of the exact wide array reads: the plan's copy or the wide array's own.
const int32_t* refit_wide_src(const mrt_tracer* t);

}  // namespace mrt
