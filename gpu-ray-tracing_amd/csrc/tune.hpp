// tune.hpp — the launch-schedule autotuner (cfg.autotune): the fixed rule, the
// candidate table, the per-key state machine and the per-handle table of settled
// schedules. Plain C++ with no HIP in it: it consumes "candidate c took x ms" and
// answers "launch candidate c next, timed or not"; mrt_api.cpp owns the events that
// measure the times (TuneEvents, tracer.hpp). tests/cpp/tune_driver.cpp runs it on the CPU.
// The limits a schedule must respect are read where they are defined: kMaxQueues
// (trace_limits.hpp), kMaxBackfill (launch_plan.hpp), the deal's block range (deal_common.hpp).
#pragma once

#include <cstdint>
#include <map>
#include <utility>

#include "../../include/mrt.h"
#include "deal_common.hpp"
#include "launch_plan.hpp"
#include "trace_limits.hpp"

namespace mrt {

// The speculative traversal turns to its leaves once at most two lanes of the
// wave still search for one, instead of waiting for the last lane (reference
// kepler_dynamic_fetch.cu:300-315): +3...+9 % on primary, diffuse and AO batches,
// -3 % on AO 1280x960 (profiles/round2_tuning.md).
constexpr int kDefaultSpecSlack = 2;
// The frontier tail (trace_kernel.hip frontier_tail): a wave that cannot refill and is
// down to at most this many live lanes finishes them 64/R lanes per ray. On by default:
// hairball diffuse 640x480 0.314 -> 0.225 ms, Mori AO 0.055 -> 0.044, bunny primary
// +5 %; conference AO and sponza diffuse lose 2-4 % (profiles/round3_frontier_ab.txt),
// where the autotuner's stage 2 can turn it off.
#ifndef MRT_DEFAULT_TAIL_LANES
#define MRT_DEFAULT_TAIL_LANES 16
#endif
constexpr int kDefaultTailLanes = MRT_DEFAULT_TAIL_LANES;
// Static strided rounds: 20 waves/CU (5 per SIMD). More resident waves evict
// each other's nodes and triangles from the vector L1 (28 waves/CU: hairball
// -22 %, profiles/round2_tuning.md); the register budget of the 4-wide kernels
// is sized for exactly this occupancy.
constexpr int kStridedWaves = 20;
constexpr int kSecondaryKey = 512;   // tuning keys only: variant | kSecondaryKey for MRT_TRACE_SECONDARY batches

// The launch configuration a trace uses (the fixed rule): the tracer's, except for a
// BVH above the Infinity Cache with every ray-distribution knob at its default.
mrt_launch_cfg effective_cfg(const mrt_launch_cfg& user, int numCUs, int64_t bvhBytes, int numRays);

// Launch-schedule autotuning state of one (batch size, kernel variant).
struct TuneState {
    // Stage 1: kSchedules ray-distribution schedules; stage 2: the stage-1 winner and
    // the runner-up, each with the speculation slack at 4 and 6, without the frontier
    // tail (with it if the tracer's default is off), with 16 lane groups, and with 2
    // lane groups at slack 6 (candidates kSchedules .. + kStage2 - 1 modify the winner,
    // the next kStage2 the runner-up; a settled choice is stored canonically as modifier
    // kSchedules + k of the schedule it modifies, so saved tables keep their meaning).
    // Stage 3: the stage-2 winner's modifier on each other schedule (kStage3 candidates from
    // kStage3First): e.g. 16 lane groups paid off at 16 waves/CU though the two stage-1 leaders
    // were 20 and 12 waves/CU (bunny primary 640x480).
    static constexpr int kSchedules = 8;
    static constexpr int kStage2 = 5;
    static constexpr int kStage3First = kSchedules + 2 * kStage2;
    static constexpr int kStage3 = kSchedules - 2;
    static constexpr int kCandidates = kStage3First + kStage3;
    static constexpr int kSamples = 8;   // timed launches per candidate; the median ranks them
    // A candidate runs kRun consecutive launches at a time, the first untimed: a launch right
    // after another schedule's inherits its cache and queue state (round 6: one launch per
    // candidate ranked a 42-us batch's schedules 3.5 % off their steady-state order).
    static constexpr int kRun = 4;
    static constexpr int kSlots = 16;    // launches in flight with a timing (back-to-back launches complete later)
    int launches = 0;    // exploring launches so far (the first round of candidates runs untimed:
                         // the clocks and caches are still settling)
    int runPos = 0;      // position of the next launch in its candidate's run
    float times[kCandidates][kSamples];
    int samples[kCandidates] = {};
    int next = 0;        // candidate the next exploring launch uses
    int rule = 0;        // the candidate equal to the fixed rule (effective_cfg) for this batch
    int stage1 = -1;     // the stage-1 winner, once every schedule has kSamples samples (once locked:
                         // the schedule the locked modifier applies to)
    int stage1b = -1;    // the stage-1 runner-up (stage 2 modifies it too; VERDICT r5 #4: the headline's
                         // saved schedule is the 8-waves/CU schedule with 2 lane groups, whose base
                         // alone loses to 20 waves/CU in stage 1)
    int stage2 = -1;     // the stage-2 pick (a modifier of stage1 or stage1b), once stage 2's have kSamples
    int s3mod = -1;      // its modifier k, tried on the schedules in s3sched (stage 3)
    int s3sched[kStage3] = {};
    int locked = -1;     // the chosen candidate (canonical: kSchedules + k of stage1), once settled
    // A saved schedule's backfilled grid (launch_plan.hpp), reached by import only (the exploring
    // stages never set them): rays per lane the grid is sized for (0: the persistent grid) and the
    // residency cap in workgroups per CU (0: the schedule's own waves/CU). Static schedules only.
    int backfill = 0;
    int capBlocks = 0;
    // and its one-shot kernel (cfg.oneshot, only with backfill 1) with its deal (cfg.deal_block):
    // by import only, like the backfill
    int oneshot = 0;
    int dealBlock = 0;
    const void* stream = nullptr;    // the stream this batch size was first launched on (only compared)
    bool multiStream = false;        // launched on several streams: not explored (settled schedule or the rule)
    bool inherited = false;          // took a nearby batch size's schedule (kTuneInherit): not exported
    int slotCand[kSlots];            // timing slot s: the candidate it times, -1 = free
    struct TuneEvents* events = nullptr;   // the slots' event pairs: the launching side's (mrt_api.cpp), opaque here

    TuneState();
    float median(int c) const;
    // The schedule and modifier (-1: none) of candidate c.
    void decode(int c, int* sched, int* mod) const;
    // Slot s finished in ms / gave no time: the slot is free again.
    void slot_done(int s, float ms);
    void slot_dropped(int s) { slotCand[s] = -1; }
    // After the finished slots were fed in: the candidate the next launch uses, and the free slot
    // its timing goes into (-1: an untimed launch). The slot is taken by slot_started, once the
    // launch is enqueued with its events around it.
    int next_launch(int* slot);
    void slot_started(int s, int cand) { slotCand[s] = cand; }
    // mrt_trace_info.autotune_candidate of a launch of candidate c; mrt_tuned_schedule.candidate once locked.
    int info_code(int c) const;
    int export_code() const;
    // mrt_tuned_schedule.candidate: the locked candidate (bits 0-7), the schedule it modifies (8-15),
    // the backfill k (16-22, at most kMaxBackfill), one-shot (23), the residency cap (24-26) and the
    // one-shot deal's block log2 (27-30: 0 or deal::kMinBlockLog2..kMaxBlockLog2 = 6..15); bit 31 zero.
    // A code from before the one-shot bits has them zero and means what it meant.
    static constexpr int kBackfillShift = 16, kOneshotShift = 23, kCapShift = 24, kDealShift = 27, kCodeBits = 31;

private:
    int pick(int incumbent, int first, int last) const;
    void settle();
};

// The launch configuration of candidate c over `base` (the rule's configuration) on a device of
// numXccs XCDs; st = null: c is a stage-1 schedule.
mrt_launch_cfg tune_candidate(int numXccs, const mrt_launch_cfg& base, int c, const TuneState* st);
// The candidate (row 0, 3 or 4 of tune_candidate's table) equal to the rule's configuration.
int rule_candidate(const mrt_launch_cfg& rule);

// The tuning states of one tracer handle, keyed (numRays, variant | kSecondaryKey for secondary rays).
struct TuneTable {
    std::map<std::pair<int, int>, TuneState*> tunes;

    // The state a launch tunes with, created (or inheriting a nearby settled size's schedule) on a
    // key's first launch; null when the launch is not eligible (autotune off, a distribution knob
    // set, MRT_TRACE_STATS), the table is full, or the key is unsettled and used on several streams:
    // the launch then runs `rule`. `user` is the tracer's configuration, `rule` effective_cfg's.
    TuneState* lookup(const mrt_launch_cfg& user, const mrt_launch_cfg& rule, uint32_t flags, int numRays, int variant,
                      const void* stream);
    // mrt_tracer_tune_export / _import (MRT_OK, MRT_ERR_INVALID_ARG: a bad entry, nothing imported,
    // MRT_ERR_TOO_LARGE: more keys than the table holds).
    int export_schedules(mrt_tuned_schedule* out, int capacity) const;
    int import_schedules(const mrt_tuned_schedule* in, int count);
    void clear();   // deletes the states (their events first, by the owner)
};

}  // namespace mrt
