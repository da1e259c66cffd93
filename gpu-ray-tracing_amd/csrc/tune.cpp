// tune.cpp — launch-schedule autotuning (cfg.autotune), see tune.hpp. No HIP here.
//
// The ray-distribution schedule that wins depends on the frame: on how the
// expensive rays fall on the static rounds, on the ray length and on the BVH's
// cache residency (profiles/round2_tuning.md: static rounds, fewer waves, per-XCD
// queues and the global queue each win somewhere by 5-70 %). With cfg.autotune
// and the distribution knobs at their defaults, the first launches of a batch
// size cycle through these eight candidates, each timed with an event pair that is
// read back on a later launch (never blocking); after kSamples launches each the
// fastest and the runner-up are timed again, each with the stage-2 modifiers (the
// speculation slack at 4 and 6, the tail toggled, 16 lane groups, 2 lane groups at
// slack 6), and the fastest is kept for that batch size. Closest hits are the same hits under
// every schedule, except that which of two triangles at exactly the same t wins follows the
// traversal order, and so can the hit an any-hit ray reports (any valid hit). A
// reproducible run pins the schedule: autotune 0, or the schedules saved per BVH
// (mrt_tracer_tune_export / _import, mrt/tuned_schedules.json for the bench).
#include "tune.hpp"

#include <algorithm>
#include <cstdlib>

namespace mrt {
namespace {

// The launch configuration a trace uses: the tracer's, except that with every
// ray-distribution knob at its default a batch over a BVH that does not fit the
// 256 MB Infinity Cache runs on one global ray queue with refills at 48 live
// lanes. Its rays are long (HBM-latency bound), so the refill atomics are rare,
// and dynamic fetch evens out the per-lane sequences whose static imbalance
// otherwise leaves much of a launch with a decaying number of live lanes. Small
// batches (at most 3 rays per lane of a 16-wave grid) get 12 waves/CU, so that even
// they refill; larger ones 16. Measured (profiles/round2_tuning.md): hairball
// diffuse 640x480 0.365 -> 0.301 ms, primary 1024x768 0.72 -> 0.42 ms, diffuse
// 1920x1080 1.04 -> 0.82 ms. Cache-resident batches keep the static strided
// rounds: there the same queue costs up to 2.6x (contended atomics).
constexpr int64_t kMallBytes = 256ll << 20;
constexpr int kBigQueueThreshold = 48;
#ifndef MRT_BIG_QUEUE_WAVES
#define MRT_BIG_QUEUE_WAVES 16
#endif
constexpr int kBigQueueWaves = MRT_BIG_QUEUE_WAVES;
constexpr int kBigQueueWavesSmall = 12;
constexpr int kBigQueueSmallRaysPerLane = 3;   // of the 16-wave grid

// Lane groups the autotuner's stage 2 tries (profiles/round3_lanegroups.txt).
constexpr int kTunedLaneGroups = 16;
// What the autotuner's stage 2 tries when tail_lanes is left at its default (16: off).
constexpr int kTunedTailLanes = 16;

constexpr int kMaxTuned = 64;   // batch sizes tuned per handle; others use the rule
constexpr int64_t kTuneInherit = 32;   // a new batch size within 1/32 of a settled one takes its schedule
// Candidate 2's per-XCD queue blocks (rays), shared tail (%) and refill threshold. No shared tail: on a
// frame in pixel order it bought 0.6 %, and on a buffer ordered costly-first (the strong-scaling shards,
// mrt.dist priority) its last rays retire at once and every XCD's waves then contend for one queue head
// (T_1 3.44 -> 3.20 ms, 8-rank shards 0.490 -> 0.445 ms without it; profiles/round4_shared_queue.txt).
constexpr int kXcdQueueBlock = 8192;
constexpr int kXcdQueueShared = 0;
constexpr int kXcdQueueThreshold = 56;

// A candidate replaces the incumbent (the fixed rule in stage 1, the stage-1 winner
// in stage 2) only when its median is this much faster: candidates within a few
// per cent of each other no longer settle differently from run to run.
constexpr float kTuneMargin = 0.03f;

}  // namespace

mrt_launch_cfg effective_cfg(const mrt_launch_cfg& user, int numCUs, int64_t bvhBytes, int numRays) {
    mrt_launch_cfg c = user;
    const bool defaults = c.num_queues < 0 && c.waves_per_cu == 0 && c.fetch_threshold == 0 && c.lane_groups == 1 &&
                          c.backfill == 0;   // a backfilled grid runs the static rounds only
    if (defaults && bvhBytes > kMallBytes) {
        const int64_t lanes16 = (int64_t)std::max(1, numCUs) * kBigQueueWaves * 64;
        c.num_queues = 1;
        c.fetch_threshold = kBigQueueThreshold;
        c.waves_per_cu = (int64_t)numRays <= kBigQueueSmallRaysPerLane * lanes16 ? kBigQueueWavesSmall : kBigQueueWaves;
    }
    return c;
}

int rule_candidate(const mrt_launch_cfg& rule) {
    return rule.num_queues == 1 ? (rule.waves_per_cu == kBigQueueWaves ? 3 : 4) : 0;
}

namespace {
mrt_launch_cfg explored_candidate(int numXccs, const mrt_launch_cfg& base, int c, const TuneState* st);
}

mrt_launch_cfg tune_candidate(int numXccs, const mrt_launch_cfg& base, int c, const TuneState* st) {
    mrt_launch_cfg x = explored_candidate(numXccs, base, c, st);
    if (st && st->backfill > 0 && st->locked >= 0 && c == st->locked) {
        // a saved schedule with a backfilled grid (imported; static schedules only): the locked
        // candidate's configuration with the grid sized for `backfill` rays per lane and, with a
        // cap, that many workgroups resident per CU
        x.backfill = st->backfill;
        if (st->capBlocks > 0) x.waves_per_cu = 4 * st->capBlocks;
        x.oneshot = st->oneshot;
        x.deal_block = st->dealBlock;
    }
    return x;
}

namespace {
// The configuration of a candidate the exploring stages reach.
mrt_launch_cfg explored_candidate(int numXccs, const mrt_launch_cfg& base, int c, const TuneState* st) {
    int sched = c, k = -1;
    if (st) st->decode(c, &sched, &k);
    if (k >= 0) {
        // stage 2/3: a schedule with the wave turning to its leaves once <= 4 (6)
        // lanes still search, with the frontier tail toggled, or with its lanes taking rays from 16
        // distant parts of each strided chunk (only for knobs the caller left at their defaults)
        mrt_launch_cfg x = explored_candidate(numXccs, base, sched, nullptr);
        if (k < 2 && base.spec_slack == kDefaultSpecSlack) x.spec_slack = k == 0 ? 4 : 6;
        if (k == 2 && base.tail_lanes == kDefaultTailLanes) x.tail_lanes = kDefaultTailLanes ? 0 : kTunedTailLanes;
        // lane groups mix a wave's rays from distant image regions: fewer waves hold a whole
        // tile of expensive rays (a silhouette), so more of them reach the frontier tail early
        // (bunny primary 640x480 0.086 -> 0.069 ms, sponza diffuse +8 %; conference AO -7 %)
        if (k == 3) x.lane_groups = kTunedLaneGroups;
        // two lane groups with slack 6: the coherent primary batches keep most of their tile
        // coherence and still shed their expensive half-tiles early (bunny primary 1024x768
        // +3 %, profiles/round4_head_knobs.txt)
        if (k == 4 && base.lane_groups == 1 && base.spec_slack == kDefaultSpecSlack) {
            x.lane_groups = 2;
            x.spec_slack = 6;
        }
        return x;
    }
    mrt_launch_cfg x = base;
    x.fetch_threshold = 0;
    x.waves_per_cu = 0;
    x.num_queues = -1;
    x.queue_block = 0;
    x.queue_shared = 0;
    switch (sched) {
        case 0: break;                                                      // static rounds, 20 waves/CU
        case 1: x.waves_per_cu = 8; break;                                  // static rounds, fewer waves
        case 2:   // per-XCD queues of 8192-ray blocks dealt cyclically (every XCD samples the whole frame,
                  // its L2 holds its own blocks' nodes and triangles), no shared tail queue,
                  // refills at 56 live lanes, 20 waves/CU: a multi-million-ray launch over a BVH above the
                  // Infinity Cache (hairball 2 M rays: 0.630 -> 0.547 ms, fabric bytes 1.07 -> 0.74 GB at
                  // 4096-ray blocks, profiles/round4_queue_ab.txt; 8192: 1.4 % faster again and the
                  // strong-scaling shards' best, round4_order_sweep.txt)
            x.num_queues = std::max(1, std::min(numXccs, kMaxQueues));   // one per XCD, never more
            x.queue_block = kXcdQueueBlock;
            x.queue_shared = kXcdQueueShared;
            x.fetch_threshold = kXcdQueueThreshold;
            x.waves_per_cu = kStridedWaves;
            break;
        case 3: x.num_queues = 1; x.fetch_threshold = kBigQueueThreshold; x.waves_per_cu = kBigQueueWaves; break;   // global queue
        case 4: x.num_queues = 1; x.fetch_threshold = 48; x.waves_per_cu = 12; break;
        case 5: x.waves_per_cu = 16; break;
        case 6: x.waves_per_cu = 12; break;
        default:   // the global queue at full occupancy: a lone multi-million-ray launch over a BVH
                   // above the Infinity Cache (hairball 2 M rays 0.728 -> 0.712 ms), whose frontier
                   // tail drains it; slower when launches overlap on two streams (the rule's 16)
            x.num_queues = 1;
            x.fetch_threshold = kBigQueueThreshold;
            x.waves_per_cu = kStridedWaves;
            break;
    }
    return x;
}
}  // namespace

TuneState::TuneState() { std::fill(slotCand, slotCand + kSlots, -1); }

float TuneState::median(int c) const {
    float v[kSamples];
    const int n = std::min(samples[c], kSamples);
    std::copy(times[c], times[c] + n, v);
    std::sort(v, v + n);
    return n ? (n % 2 ? v[n / 2] : 0.5f * (v[n / 2 - 1] + v[n / 2])) : 1e30f;
}

// Stage 1 a schedule, stage 2 a modifier of the stage-1 winner or runner-up, stage 3 the
// stage-2 modifier on another schedule. A settled candidate is canonical: kSchedules + k
// modifies stage1.
void TuneState::decode(int c, int* sched, int* mod) const {
    if (c < kSchedules) {
        *sched = c;
        *mod = -1;
    } else if (c < kStage3First) {
        const bool second = c >= kSchedules + kStage2;
        *sched = second ? stage1b : stage1;
        *mod = (c - kSchedules) % kStage2;
    } else {
        *sched = s3sched[c - kStage3First];
        *mod = s3mod;
    }
}

// stage-2 candidates (another speculation slack) carry their stage-1 schedule in bits 8+
// canonical: a modifier k of the schedule it modifies, kSchedules + k | schedule << 8
int TuneState::info_code(int c) const {
    int sched = c, mod = -1;
    decode(c, &sched, &mod);
    return mod >= 0 ? (kSchedules + mod) | (sched << 8) : c;
}

// candidate field: the locked candidate | the stage-1 winner << 8 (stage-2 candidates
// are the stage-1 schedule with another speculation slack)
int TuneState::export_code() const {
    return locked | (std::max(0, stage1) << 8) | (backfill << kBackfillShift) | (capBlocks << kCapShift) |
           (oneshot << kOneshotShift) | (dealBlock << kDealShift);
}

int TuneState::pick(int incumbent, int first, int last) const {
    int best = incumbent;
    for (int c = first; c < last; c++)
        if (c != incumbent && median(c) < median(best)) best = c;
    return median(best) < (1.0f - kTuneMargin) * median(incumbent) ? best : incumbent;
}

void TuneState::slot_done(int s, float ms) {
    const int c = slotCand[s];
    if (samples[c] < kSamples) times[c][samples[c]++] = ms;
    slotCand[s] = -1;
}

// The stage whose candidates all have kSamples samples ends: its pick is the next stage's
// incumbent, or the settled choice.
void TuneState::settle() {
    auto sampled = [&](int first, int last) {
        for (int c = first; c < last; c++)
            if (samples[c] < kSamples) return false;
        return true;
    };
    if (stage1 < 0) {
        if (!sampled(0, kSchedules)) return;
        stage1 = pick(rule, 0, kSchedules);
        for (int c = 0; c < kSchedules; c++)
            if (c != stage1 && (stage1b < 0 || median(c) < median(stage1b))) stage1b = c;
        next = kSchedules;
        runPos = 0;
        return;
    }
    if (stage2 < 0) {
        if (!sampled(kSchedules, kStage3First)) return;
        samples[stage1] = std::min(samples[stage1], kSamples);
        const int p = pick(stage1, kSchedules, kStage3First);
        if (p < kSchedules) {   // no modifier beats the stage-1 winner: settled
            locked = p;
            return;
        }
        int sched, mod;
        decode(p, &sched, &mod);
        stage2 = p;
        s3mod = mod;
        for (int c = 0, i = 0; c < kSchedules; c++)
            if (c != stage1 && c != stage1b) s3sched[i++] = c;
        next = kStage3First;
        runPos = 0;
        return;
    }
    if (!sampled(kStage3First, kCandidates)) return;
    const int p = pick(stage2, kStage3First, kCandidates);
    int sched, mod;
    decode(p, &sched, &mod);
    stage1 = sched;   // canonical: modifier kSchedules + mod of schedule stage1
    locked = kSchedules + mod;
}

int TuneState::next_launch(int* slot) {
    *slot = -1;
    if (locked < 0) settle();
    if (locked >= 0) return locked;
    // runs of kRun launches per candidate, cycling over the current stage's candidates;
    // the first launch of a run (and the whole first cycle of stage 1) is untimed
    const int cand = next;
    const bool timed = runPos > 0 && launches >= kSchedules * kRun;
    launches++;
    if (++runPos == kRun) {
        runPos = 0;
        const int first = stage1 < 0 ? 0 : (stage2 < 0 ? kSchedules : kStage3First);
        const int last = stage1 < 0 ? kSchedules : (stage2 < 0 ? kStage3First : kCandidates);
        next = first + (next + 1 - first) % (last - first);
    }
    if (timed)
        for (int s = 0; s < kSlots; s++)
            if (slotCand[s] < 0) {
                *slot = s;
                break;
            }
    return cand;
}

TuneState* TuneTable::lookup(const mrt_launch_cfg& uc, const mrt_launch_cfg& rule, uint32_t flags, int numRays,
                             int variant, const void* stream) {
    if (!(uc.autotune && uc.num_queues < 0 && uc.waves_per_cu == 0 && uc.fetch_threshold == 0 && uc.lane_groups == 1 &&
          uc.backfill == 0 && uc.oneshot == 0 && uc.deal_block == 0 && !(flags & MRT_TRACE_STATS)))
        return nullptr;
    // secondary rays (MRT_TRACE_SECONDARY) settle their own schedule: a diffuse batch of a primary
    // batch's size runs differently (round-5 README table: Mori primary 4829 Mrays/s on the diffuse
    // batch's schedule, 5814 on its own)
    const auto key = std::make_pair(numRays, variant | ((flags & MRT_TRACE_SECONDARY) ? kSecondaryKey : 0));
    TuneState* tune = nullptr;
    auto it = tunes.find(key);
    if (it != tunes.end()) {
        tune = it->second;
    } else if ((int)tunes.size() < kMaxTuned) {
        tune = new TuneState();
        tune->stream = stream;
        tune->rule = rule_candidate(rule);
        // A batch within 1/kTuneInherit of a settled batch size of the same variant takes
        // that schedule instead of exploring (the nearest one): the strong-scaling shards of
        // one frame differ by a block or two (2,064,384 .. 2,080,768 rays against the saved
        // 2,073,600), and the exploring launches of every shard size would fall in the timed steps:
        // kRun * kSchedules untimed, then kRun * n * C - (kRun - 1 - r) per stage of n = kSchedules,
        // 2 * kStage2, kStage3 candidates (C = ceil(kSamples / (kRun - 1)) cycles, the last run cut
        // after its r = kSamples - (C - 1) * (kRun - 1) timed launches): 246 without stage 3, 317
        // with it (tests/test_tune.py), plus the in-flight lag of asynchronous launches (256-328
        // measured, profiles/round6_autotune_vs_saved.json).
        int64_t bestGap = -1;
        for (const auto& kv : tunes) {
            if (kv.first.second != key.second || kv.second->locked < 0) continue;
            const int64_t gap = std::llabs((int64_t)kv.first.first - numRays);
            if (gap * kTuneInherit > (int64_t)kv.first.first || (bestGap >= 0 && gap >= bestGap)) continue;
            bestGap = gap;
            tune->stage1 = kv.second->stage1;
            tune->locked = kv.second->locked;
            tune->backfill = kv.second->backfill;
            tune->capBlocks = kv.second->capBlocks;
            tune->oneshot = kv.second->oneshot;
            tune->dealBlock = kv.second->dealBlock;
            tune->inherited = true;
        }
        tunes[key] = tune;
    }
    // A batch size launched on several streams is not explored there: its launches
    // overlap, and a candidate's time alone no longer ranks the pipeline. It runs its
    // settled schedule (saved, inherited, or settled on one stream) if it has one, else
    // the fixed rule (the bench's two-stream hairball 8 spp buffer: 4.23 ms on the rule,
    // 3.48 on the per-XCD block-cyclic schedule).
    if (tune && !tune->stream) tune->stream = stream;   // an imported schedule: first used here
    if (tune && tune->stream != stream) tune->multiStream = true;
    if (tune && tune->multiStream && tune->locked < 0) tune = nullptr;
    return tune;
}

int TuneTable::export_schedules(mrt_tuned_schedule* out, int capacity) const {
    int n = 0;
    for (const auto& kv : tunes) {
        // inherited entries were tuned for another batch (size and ray distribution): not saved as tuned
        if (kv.second->locked < 0 || kv.second->inherited) continue;
        if (n < capacity) out[n] = mrt_tuned_schedule{kv.first.first, kv.first.second, kv.second->export_code(), MRT_TUNE_VERSION};
        n++;
    }
    return n;
}

int TuneTable::import_schedules(const mrt_tuned_schedule* in, int count) {
    for (int i = 0; i < count; i++) {
        const int code = in[i].candidate;
        if (code < 0 || (code >> TuneState::kCodeBits) != 0) return MRT_ERR_INVALID_ARG;
        const int locked = code & 0xff, stage1 = (code >> 8) & 0xff;
        const int backfill = (code >> TuneState::kBackfillShift) & 0x7f, cap = (code >> TuneState::kCapShift) & 7;
        const int oneshot = (code >> TuneState::kOneshotShift) & 1, block = (code >> TuneState::kDealShift) & 15;
        if (in[i].version != MRT_TUNE_VERSION || in[i].num_rays <= 0 || locked >= TuneState::kSchedules + TuneState::kStage2 ||
            stage1 >= TuneState::kSchedules || backfill > kMaxBackfill || (cap > 0 && backfill == 0))
            return MRT_ERR_INVALID_ARG;
        // one-shot is a grid of one ray per lane; the deal's blocks are the one-shot kernels'
        if ((oneshot && backfill != 1) ||
            (block != 0 && (!oneshot || block < deal::kMinBlockLog2 || block > deal::kMaxBlockLog2)))
            return MRT_ERR_INVALID_ARG;
        // a backfilled grid is for the static schedules only: no workgroup of theirs waits for another
        const int sched = locked < TuneState::kSchedules ? locked : stage1;
        if (backfill > 0 && tune_candidate(1, mrt_launch_cfg{}, sched, nullptr).num_queues >= 1) return MRT_ERR_INVALID_ARG;
    }
    for (int i = 0; i < count; i++) {
        const auto key = std::make_pair((int)in[i].num_rays, (int)in[i].variant);
        auto it = tunes.find(key);
        if (it == tunes.end()) {
            if ((int)tunes.size() >= kMaxTuned) return MRT_ERR_TOO_LARGE;
            it = tunes.emplace(key, new TuneState()).first;
        }
        it->second->stage1 = (in[i].candidate >> 8) & 0xff;
        it->second->locked = in[i].candidate & 0xff;
        it->second->backfill = (in[i].candidate >> TuneState::kBackfillShift) & 0x7f;
        it->second->capBlocks = (in[i].candidate >> TuneState::kCapShift) & 7;
        it->second->oneshot = (in[i].candidate >> TuneState::kOneshotShift) & 1;
        it->second->dealBlock = (in[i].candidate >> TuneState::kDealShift) & 15;
        it->second->inherited = false;   // a schedule saved for this very key: exported again
    }
    return MRT_OK;
}

void TuneTable::clear() {
    for (auto& kv : tunes) delete kv.second;
    tunes.clear();
}

}  // namespace mrt
