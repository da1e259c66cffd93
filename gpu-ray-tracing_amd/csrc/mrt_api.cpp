// mrt_api.cpp — the C-ABI of include/mrt.h: per-device tracer contexts (tracer.hpp), their
// launch configuration, the workspace pool (queue heads, stack spill slab), the events that time
// the autotuner's launches (its policy: tune.cpp) and the trace path with its persistent-grid
// sizing. Bind and the 4-wide derivation: bind_api.cpp; refit: refit_api.cpp; the device build:
// build_api.cpp; the reference-compatible entry points of CudaTracerKernels.hh:42-52: compat_api.cpp.
//
// The library never owns the caller's BVH/ray/result buffers (reference
// ownership: CudaBVH.cc:101-109, RayBuffer.cc:42-81). It owns only its
// workspace, sized for the persistent grid it launches.
#include <algorithm>
#include <cstring>
#include <string>

#include "launch_plan.hpp"
#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;
using mrt::hipFail;

namespace mrt {
namespace {
thread_local std::string g_lastError;
}  // namespace

// Shared with every other C-ABI file (through api_common.hpp's fail).
int api_fail(int code, const std::string& what) {
    g_lastError = what;
    return code;
}
const char* api_last_error() { return g_lastError.c_str(); }

namespace {
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

// Both events of a pair, or none: a pair is never left half made.
int create_pair(EventPair* out, unsigned startFlags, unsigned stopFlags) {
    EventPair p;
    MRT_HIP(p.start.create(startFlags));
    MRT_HIP(p.stop.create(stopFlags));
    *out = std::move(p);
    return MRT_OK;
}
}  // namespace
}  // namespace mrt

namespace {

// The frontier tail runs in the exact 4-wide kernels whose leaf refs carry counts.
bool with_tail(const mrt_tracer* t, const mrt::TraceVariant& v, const mrt_launch_cfg& c) {
    return c.tail_lanes > 0 && v.nodes == mrt::kNodeWide4 && t->wide.leafCounts;
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
    v.nodes = (t->cfg.wide != 0 && t->wide.nodes && v.speculative) ? t->wide.format : mrt::kNodeCompact2;
    v.tail = with_tail(t, v, t->cfg);
    return v;
}

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

// The variant a kernel_key names; false where the key's stack or node-format field has no meaning.
bool variant_of_key(int key, mrt::TraceVariant* v) {
    const int lds = (key >> 4) & 3, nodes = (key >> 6) & 3;
    if (key < 0 || key >= 1024 || lds > 2 || nodes > mrt::kNodeWide4Q) return false;
    v->anyHit = (key & 1) != 0;
    v->speculative = (key & 2) != 0;
    v->exactRcp = (key & 4) != 0;
    v->stats = (key & 8) != 0;
    v->ldsStack = 8 << lds;
    v->nodes = nodes;
    v->tail = (key & 256) != 0;
    v->oneshot = (key & 512) != 0;
    return true;
}

// The kernel function a key's variant launches (null: none), and the reverse: the smallest key
// whose variant launches `fn` (-1: none). By the function, not by the variant asked for, so a
// dispatcher that serves one variant with a sibling's kernel shows (mrt_tracer_last_kernel_key).
const void* kernel_of_key(int key) {
    mrt::TraceVariant v{};
    return variant_of_key(key, &v) ? mrt::trace_kernel_function(v) : nullptr;
}

int key_of_kernel(const void* fn) {
    for (int key = 0; fn && key < 1024; key++)
        if (kernel_of_key(key) == fn) return key;
    return -1;
}

// Workgroups per CU the code object of a variant admits (queried once).
int variant_occupancy(mrt_tracer* t, const mrt::TraceVariant& v) {
    int& occ = t->occ[kernel_key(v)];
    if (occ <= 0 && (mrt::trace_occupancy(v, &occ) != hipSuccess || occ <= 0)) occ = 1;
    return occ;
}

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

// The grid of kernel v (launch_plan.hpp): the persistent one — as many 256-thread workgroups per CU
// as the config asks for (or the batch size suggests) and the code object's occupancy admits,
// every workgroup resident at once — or, with cfg.backfill, one sized from the batch.
mrt::LaunchPlan kernel_plan(mrt_tracer* t, const mrt_launch_cfg& cfg, const mrt::TraceVariant& v, int numRays, int stackCap) {
    mrt::LaunchPlanIn in;
    in.numRays = numRays;
    in.numCUs = t->numCUs;
    in.blockThreads = mrt::kBlockThreads;
    in.wavesPerCU = mrt::grid_waves_per_cu(t->numCUs, cfg, numRays);
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

// The launch's grid and the kernel it is for (v->oneshot). cfg.oneshot: the one-shot sibling on the
// grid planned for it; where the variant has none, the batch fits the resident grid or the slab cap
// asks for more than one ray per lane, today's kernel and plan.
mrt::LaunchPlan launch_plan(mrt_tracer* t, const mrt_launch_cfg& cfg, mrt::TraceVariant* v, int numRays, int stackCap) {
    v->oneshot = cfg.oneshot == 1 && cfg.backfill == 1 && mrt::trace_has_oneshot(*v);
    mrt::LaunchPlan plan = kernel_plan(t, cfg, *v, numRays, stackCap);
    if (v->oneshot && !plan.oneshot) {
        v->oneshot = false;
        plan = kernel_plan(t, cfg, *v, numRays, stackCap);
    }
    return plan;
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

// The scratch of `stream`: its own set, else a new one, else (kMaxWorkspaces
// reached) the least recently used set once its last launch has completed —
// grown to the grid's spill slab.
int workspace_for(mrt_tracer* t, void* stream, int totalLanes, int ldsStack, int stackCap, mrt::Workspace** out) {
    mrt::Workspace* w = nullptr;
    for (const auto& x : t->workspaces)
        if (x->stream == stream) w = x.get();
    if (!w && (int)t->workspaces.size() >= mrt::kMaxWorkspaces) {
        for (const auto& x : t->workspaces)
            if (!w || x->lastUse < w->lastUse) w = x.get();
        if (int rc = workspace_wait(w)) return rc;   // its previous stream's launch may still run
        w->stream = stream;
    }
    if (!w) {
        // made completely before it is listed: a failed allocation leaves no set behind
        auto fresh = std::make_unique<mrt::Workspace>();
        fresh->stream = stream;
        MRT_HIP(fresh->queues.alloc(mrt::kQueueLines * mrt::kQueueStrideWords * sizeof(unsigned)));
        MRT_HIP(fresh->status.alloc(64 * sizeof(int)));
        MRT_HIP(hipMemset(fresh->status.get(), 0, 64 * sizeof(int)));
#ifdef MRT_DONE_EVENT
        MRT_HIP(fresh->done.create(mrt::kDoneEventFlags));
#endif
        w = fresh.get();
        t->workspaces.push_back(std::move(fresh));
    }
    w->lastUse = ++t->useClock;
    const size_t need = (size_t)(stackCap - ldsStack) * (size_t)totalLanes;
    if (need > w->spillInts) {
        // A smaller slab may still be in use by this scratch's previous launch.
        if (int rc = workspace_wait(w)) return rc;
        w->spillInts = 0;
        MRT_HIP(w->spill.free());
        MRT_HIP(w->spill.alloc(need * sizeof(int)));
        w->spillInts = need;
    }
    if (!t->blocking.start) {
        // the blocking call's timing pair: no system-scope fence around the kernel (it would
        // flush the caches and be timed with it); the stop event releases to device scope,
        // so the overflow count read after it is current
        if (int rc = mrt::create_pair(&t->blocking, mrt::kTimingEventFlags, hipEventReleaseToDevice)) return rc;
    }
    *out = w;
    return MRT_OK;
}

// ---- launch-schedule autotuning (cfg.autotune): the events ----------------------
// The policy is tune.cpp's (the candidate table tune_candidate, the stages, the table of
// settled schedules); here are the event pairs that time its exploring launches.

// Feeds the timings of the launches that have completed to their state (never blocking).
void tune_collect(mrt::TuneState* st) {
    for (int s = 0; s < mrt::TuneState::kSlots; s++) {
        if (st->slotCand[s] < 0 || hipEventQuery(st->events->slot[s].stop) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, st->events->slot[s].start, st->events->slot[s].stop) == hipSuccess) st->slot_done(s, ms);
        else st->slot_dropped(s);
    }
}

// The event pair of timing slot `slot`, created on its first use.
int tune_events(mrt::TuneState* st, int slot, hipEvent_t* start, hipEvent_t* stop) {
    if (!st->events) st->events = new mrt::TuneEvents();
    mrt::EventPair& ev = st->events->slot[slot];
    if (!ev.start)
        if (int rc = mrt::create_pair(&ev, mrt::kTimingEventFlags, mrt::kTimingEventFlags)) return rc;
    *start = ev.start;
    *stop = ev.stop;
    return MRT_OK;
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
    if (!t->bvh) return fail(MRT_ERR_NOT_BOUND, "trace before bind (no BVH)");
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
    a.nodes = static_cast<const float4*>(wide ? t->wide.nodes.get() : t->bvh.nodes);
    a.woop = static_cast<const float4*>(t->bvh.woop);
    a.triIndex = t->bvh.triIndex;
    a.nodeBytes = (uint32_t)(wide ? t->wide.bytes : t->bvh.nodeBytes);
    a.woopBytes = (uint32_t)t->bvh.woopBytes;
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
    a.wideLeafCounts = wide && t->wide.leafCounts;
    a.laneGroupsLog2 = __builtin_ctz((unsigned)cfg.lane_groups);
    a.totalLanes = totalLanes;
    a.stackCap = stackCap;
    a.stackBound = wide ? t->wide.stackBound : stackCap - 1;
    a.tailLanes = cfg.tail_lanes;
    a.xccMask = cfg.queue_xcc_mask;
    a.dealBlockLog2 = v.oneshot ? cfg.deal_block : 0;
    a.raySort = cfg.ray_sort;
    a.queues = ws->queues.get();
    a.spill = ws->spill.get();
    // The blocking call counts this launch's overflows in a slot of its own; the
    // asynchronous one adds to the sticky counter (mrt_tracer_stack_overflows).
    a.status = blocking ? ws->status.get() + mrt::kTimedSlot : ws->status.get();
    return a;
}

// Enqueues the launch on s: inside the blocking call's event pair when `blocking`, and inside
// the autotuner's (tuneStart, tuneStop) when it times this launch.
int enqueue_trace(mrt_tracer* t, const mrt::TraceVariant& v, const mrt::TraceArgs& a, int blocks, int dynLds,
                  mrt::Workspace* ws, hipStream_t s, bool blocking, hipEvent_t tuneStart, hipEvent_t tuneStop) {
    // Queue heads restart at zero for every launch; strided mode has none.
    if (a.numQueues > 0)
        MRT_HIP(hipMemsetAsync(ws->queues.get(), 0, mrt::kQueueLines * mrt::kQueueStrideWords * sizeof(unsigned), s));
    if (blocking) MRT_HIP(hipMemsetAsync(ws->status.get() + mrt::kTimedSlot, 0, sizeof(int), s));
    if (blocking) MRT_HIP(hipEventRecord(t->blocking.start, s));
    if (tuneStart) MRT_HIP(hipEventRecord(tuneStart, s));
    MRT_HIP(mrt::launch_trace(v, a, blocks, s, dynLds));
    t->lastKernel = mrt::trace_kernel_function(v);
#ifdef MRT_DONE_EVENT
    MRT_HIP(hipEventRecord(ws->done, s));
#endif
    ws->launched = true;
    if (tuneStop) MRT_HIP(hipEventRecord(tuneStop, s));
    if (blocking) MRT_HIP(hipEventRecord(t->blocking.stop, s));
    return MRT_OK;
}

// The blocking call: waits for the launch and reports it (the autotune fields are the caller's).
int fill_info(mrt_tracer* t, const mrt::TraceVariant& v, const mrt::TraceArgs& a, const mrt::Workspace* ws,
              mrt_trace_info* info) {
    info->stack_capacity = a.stackCap;
    MRT_HIP(hipEventSynchronize(t->blocking.stop));
    MRT_HIP(hipEventElapsedTime(&info->kernel_ms, t->blocking.start, t->blocking.stop));
    info->grid_waves = a.totalLanes / 64;
    info->block_threads = mrt::kBlockThreads;
    info->lds_stack_entries = v.ldsStack;
    info->wide = v.nodes != mrt::kNodeCompact2 ? 4 : 2;
    info->node_bytes = v.nodes == mrt::kNodeWide4 ? 128 : 64;
    info->num_queues = a.numQueues;
    info->fetch_threshold = a.fetchThreshold;
    int overflow = 0;
    MRT_HIP(hipMemcpy(&overflow, ws->status.get() + mrt::kTimedSlot, sizeof(int), hipMemcpyDeviceToHost));
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
    mrt_launch_cfg cfg = mrt::effective_cfg(t->cfg, t->numCUs, t->bvh.nodeBytes + t->bvh.woopBytes, numRays);
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
    const int stackCap = v.nodes != mrt::kNodeCompact2 ? t->wide.stackCap : mrt::kStackCapacity;
    const mrt::LaunchPlan plan = launch_plan(t, cfg, &v, numRays, stackCap);
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

}  // namespace

namespace mrt {

int wait_all_workspaces(mrt_tracer* t) {
    for (const auto& w : t->workspaces)
        if (int rc = workspace_wait(w.get())) return rc;
    return MRT_OK;
}

void tune_reset(mrt_tracer* t) {
    for (auto& kv : t->tunes.tunes) {
        TuneEvents* ev = kv.second->events;
        // a timed launch may not have reached its stop event yet
        for (int s = 0; ev && s < TuneState::kSlots; s++)
            if (ev->slot[s].start) (void)hipEventSynchronize(ev->slot[s].stop);
        delete ev;
    }
    t->tunes.clear();
}

}  // namespace mrt

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
    mrt::DeviceBuf<unsigned long long> d;
    MRT_HIP(d.alloc(sizeof(unsigned long long)));
    hipError_t e = hipMemset(d.get(), 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = mrt::selftest_exact_rcp(d.get(), nullptr);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d.get(), sizeof(h), hipMemcpyDeviceToHost);
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
    t->cfg = mrt::default_cfg();
    *out = t;
    return MRT_OK;
}

int mrt_tracer_destroy(mrt_tracer* t) {
    if (!t) return MRT_OK;
    {
        // each owner lets go after the wait that makes it safe (unbind: event waits, the streams
        // may already be destroyed; the plan, the wide array, the tuned schedules)
        DeviceGuard guard(t->device);
        (void)mrt::unbind_locked(t);
        t->workspaces.clear();
        t->blocking = mrt::EventPair{};
    }
    delete t;
    return MRT_OK;
}

int mrt_tracer_set_config(mrt_tracer* t, const mrt_launch_cfg* cfg) {
    if (!t || !cfg) return fail(MRT_ERR_INVALID_ARG, "null argument");
    const mrt_launch_cfg c = mrt::resolve_cfg(*cfg);
    if (!mrt::valid_cfg(c)) return fail(MRT_ERR_INVALID_ARG, "launch config out of range");
    std::lock_guard<std::mutex> lock(t->mu);
    t->cfg = c;
    return mrt::refresh_wide(t, false);   // the plan and the schedules go; the wide array if cfg.wide changed
}

int mrt_tracer_get_config(const mrt_tracer* t, mrt_launch_cfg* cfg) {
    if (!t || !cfg) return fail(MRT_ERR_INVALID_ARG, "null argument");
    *cfg = t->cfg;
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

int mrt_trace_kernel_keys(int32_t* keys, int capacity) {
    int n = 0;
    for (int key = 0; key < 1024; key++) {
        // a key whose variant is served by the kernel of a smaller key has no kernel of its own
        if (!kernel_of_key(key) || key_of_kernel(kernel_of_key(key)) != key) continue;
        if (keys && n < capacity) keys[n] = key;
        n++;
    }
    return n;
}

int mrt_tracer_last_kernel_key(const mrt_tracer* t) {
    if (!t) return -1;
    std::lock_guard<std::mutex> lock(const_cast<mrt_tracer*>(t)->mu);
    return key_of_kernel(t->lastKernel);
}

int mrt_tracer_stack_overflows(mrt_tracer* t, int64_t* count, int32_t reset) {
    if (!t || !count) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    DeviceGuard guard(t->device);
    int64_t total = 0;
    for (const auto& w : t->workspaces) {
        int n = 0;
        if (int rc = workspace_wait(w.get())) return rc;
        MRT_HIP(hipMemcpy(&n, w->status.get(), sizeof(int), hipMemcpyDeviceToHost));
        total += n;
        if (reset) MRT_HIP(hipMemset(w->status.get(), 0, sizeof(int)));
    }
    *count = total;
    return MRT_OK;
}

}  // extern "C"
