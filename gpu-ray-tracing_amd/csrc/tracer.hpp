// tracer.hpp — the tracer handle behind include/mrt.h and the functions of one C-ABI file that
// another one calls. The handle's sub-objects own their device memory and events; each file
// works on its own: the handle's lifecycle, configuration, workspace pool, tune events and the
// trace path (mrt_api.cpp), refit (refit_api.cpp), the device build (build_api.cpp), the plan and
// the 4-wide array derived on the device (derive_api.cpp), the treelet restructuring
// (optimize_api.cpp). What a tracer holds of a bound tree (the borrowed buffers, the wide array
// with its source map, the refit plan) has one writer, bind_api.cpp's commit: a bind and an
// unbind replace all of it, set_config the plan, the schedules and (where cfg.wide changed) the
// wide array, optimize all but the schedules, the first refit only the plan.
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

// The bound Compact2 BVH: device pointers borrowed from the caller. The extern "C" functions
// build one from their arguments; a tracer that holds none (nodes null) is unbound.
struct BvhBuffers {
    const void* nodes = nullptr;
    int64_t nodeBytes = 0;
    const void* woop = nullptr;
    int64_t woopBytes = 0;
    const int32_t* triIndex = nullptr;
    int64_t triIndexBytes = 0;
    explicit operator bool() const { return nodes != nullptr; }
    int64_t numNodes() const { return nodeBytes / 64; }
};

// 4-wide nodes derived from the bound Compact2 tree (cfg.wide), owned by the tracer: made by
// install (a bind: the host collapse of wide_bvh.cpp, or derive_api.cpp on the device) or by
// refresh_wide (set_config changed cfg.wide; the quantized form after a refit), dropped by unbind.
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
    // Exact form only, the source map: per wide child the Compact2 slot (binary node * 2 + side)
    // its box was copied from, -1 = absent — from the collapse that produced `nodes` (a refit
    // copies the refitted boxes along it; collapsing refitted nodes again would choose other
    // children). Its one home is the device, with the array it belongs to: the device derivation
    // writes it there; the host collapse leaves it in srcHost until the tracer holds a refit plan
    // (commit uploads it then and releases srcHost), so a tracer that never refits pays nothing.
    DeviceBuf<int32_t> src;
    std::vector<int32_t> srcHost;
    int64_t srcBytes() const { return src ? bytes / 128 * 16 : 0; }
};

// Largest wide-traversal stack a tracer sizes its spill slab for (entries per lane).
constexpr int kMaxWideStack = 1024;

// The refit plan (mrt_tracer_refit): the nodes by height level and the refit's scratch, on the
// device. Installed by a device bind, build or optimize, else by the first refit after a bind or
// set_config; dropped by bind, unbind and set_config. The wide source map is not part of it
// (WideArray::src); mrt_refit_info.plan_bytes counts both.
struct RefitPlan {
    bool built = false;
    DeviceBuf<int32_t> order;      // numNodes node indices, level by level
    DeviceBuf<int32_t> offsets;    // levels + 1 offsets into order
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

// What derive() yields: the run, the plan it filled, or tooDeep (more than MRT_DERIVE_MAX_LEVELS
// depth levels: no plan, the caller takes the host path).
struct Derivation {
    DeriveRun run;
    RefitPlan plan;
    bool tooDeep = false;
};

// What commit() puts in place of what the tracer holds; a null part stays as it is.
struct Install {
    WideArray* wide = nullptr;
    RefitPlan* plan = nullptr;
    const mrt_derive_info* derive = nullptr;   // lastDerive (wall_ms: the time since `since`)
    const std::chrono::steady_clock::time_point* since = nullptr;   // with `wide`: bindMs
    bool keepTunes = false;
};
enum : unsigned { kKeepTunes = 1, kUnbindOnError = 2 };   // install()'s flags

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

    mrt_launch_cfg cfg{};

    // The bound tree and what is derived from it. commit() (bind_api.cpp) is their only writer.
    mrt::BvhBuffers bvh;
    mrt::WideArray wide;
    mrt::RefitPlan plan;
    double bindMs = 0.0;               // wall time of the last bind / wide derivation (mrt_trace_info)
    mrt_derive_info lastDerive{};      // the last device bind / build / plan (mrt_tracer_derive_info)
    mrt_build_info lastBuild{};        // the last successful mrt_tracer_build (mrt_tracer_build_info)
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

// bind_api.cpp. check_bind_args: mrt_tracer_bind's and mrt_tracer_bind_device's argument checks.
//
// commit: the one writer of t->bvh, wide, plan, bindMs and lastDerive. It first does what can
// fail (the source map goes to the device once a plan is held; this handle's traces, which read
// the wide array, and its refit, which writes it and reads the plan, have finished), then
// replaces, then forgets the tuned schedules unless told to keep them. On an error the tracer
// holds what it held; only an unbind (b empty) goes through whatever the waits said.
//
// install: a bind. Makes the wide array cfg.wide asks for (d with a plan and cfg.wide 1: on the
// device, enqueued on s, returning after the device has finished; else the host collapse) and
// commits it with b and d's plan (d null: the host route, no plan, lastDerive stays; d->tooDeep:
// the same, and lastDerive says so). since: the start of what bindMs counts (null: now).
// kUnbindOnError: the caller has written the buffers, or promises it (mrt_tracer_bind_device).
// unbind_locked is the install of nothing.
//
// refresh_wide: the host collapse again where set_config changed what cfg.wide asks for (the plan
// and the schedules go in any case), or afterRefit for the quantized form, which has no
// in-place update (plan and schedules stay). A collapse that fails leaves no array held.
int check_bind_args(const mrt_tracer* t, const BvhBuffers& b);
int commit(mrt_tracer* t, const BvhBuffers& b, const Install& in);
int install(mrt_tracer* t, const BvhBuffers& b, Derivation* d, hipStream_t s, unsigned flags,
            const std::chrono::steady_clock::time_point* since = nullptr);
int unbind_locked(mrt_tracer* t);
int refresh_wide(mrt_tracer* t, bool afterRefit);

// The levels 1 .. of a plan's host offsets, lowest first: level(begin, count) per level above
// tailNodes nodes, then tail(firstLevel, numLevels) once, in one workgroup, for all smaller ones
// (level sizes never grow with the height). Both return a hipError_t; *launches counts them.
template <class Level, class Tail>
int walk_levels(const std::vector<int64_t>& offsets, int tailNodes, int* launches, Level level, Tail tail) {
    const int levels = (int)offsets.size() - 1;
    for (int l = 1; l < levels; l++) {
        const int begin = (int)offsets[(size_t)l], count = (int)(offsets[(size_t)l + 1] - begin);
        const bool rest = count <= tailNodes;
        MRT_HIP(rest ? tail(l, levels) : level(begin, count));
        ++*launches;
        if (rest) break;
    }
    return MRT_OK;
}

// refit_api.cpp: waits for a refit that may still run (it reads the plan and writes the wide
// array); the refit's launches on Compact2 buffers, bound or not. The level plan made on the
// host, for a host build or a tree above MRT_DERIVE_MAX_LEVELS depth levels: host_levels brings
// the records to the host (a tree that is none: `code` with `prefix` + the reason),
// upload_levels writes order, offsets (levels + 1) and a cleared skipped counter into the
// caller's device buffers and returns after the copies.
struct RefitLevels;
int wait_refit(mrt_tracer* t);
int enqueue_refit(const RefitArgs& a, const std::vector<int64_t>& levelOffsets, const int32_t* order,
                  const int32_t* offsets, hipStream_t s, int* launches);
int host_levels(const void* nodes, int64_t numNodes, hipStream_t s, int code, const char* prefix, RefitLevels* lv);
int upload_levels(const RefitLevels& lv, int32_t* order, int32_t* offsets, unsigned long long* skipped, hipStream_t s);

// derive_api.cpp: the refit plan and the exact 4-wide array derived on the device (wide_kernel.hip).
// derive: the plan of `numNodes` records at `nodes` into d (order, offsets, levels, valid,
// skipped; not built), enqueued on s with a few waits; a tree that is none fails with `code` and
// `prefix` + refit_levels' reason. derive_wide: the exact array of d's tree, its boxes final,
// into w (no array where the stack bound is above kMaxWideStack). derive_report: what
// mrt_tracer_derive_info says of d's run (not wall_ms), once s has finished.
int derive(Derivation& d, const void* nodes, int64_t numNodes, hipStream_t s, int code, const char* prefix);
int derive_wide(DeriveRun& r, const BvhBuffers& b, WideArray* w, hipStream_t s);
int derive_report(const DeriveRun& r, bool plan, bool wide, mrt_derive_info* info);

}  // namespace mrt
