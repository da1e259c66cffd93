// tune_driver.cpp — runs the launch-schedule autotuner (csrc/tune.cpp) on the CPU: what
// mrt_api.cpp does around a launch (look the key up, feed the finished timings in, ask for
// the next candidate, start its timing), with a time model from the command line in place of
// the GPU. Built from this file and tune.cpp alone by the host compiler: no HIP, no libmrt.
// tests/test_tune.py reads its output.
//
//   tune_driver [--base t0,..,t7] [--mod f0,..,f4] [--pair S:K:F]... [--lag N|never]
//               [--bvh-mb M] [--cus N] [--xcds N] [--rule R] OP...
//
// A launch of schedule S with modifier K takes base[S] * mod[K] ms (--pair S:K:F: base[S] * F).
// Its timing is readable --lag launches of the same key after the next one (0: by the next
// launch, as with mrt_tracer_trace_timed; never: no launch ever completes). --rule R refuses
// a launch whose fixed rule is not candidate R (a check of --bvh-mb against the batch size).
//
//   cfg FIELD VALUE                the tracer's mrt_launch_cfg (starts at the library defaults)
//   flags N                        MRT_TRACE_* flags of the launches that follow
//   launch RAYS VARIANT STREAM [N] N launches; one line each: cand, info (autotune_candidate), locked
//   import N {RAYS VARIANT CANDIDATE VERSION}xN     export
//   schedules                      the eight stage-1 rows of tune_candidate
//   modifier S K                   tune_candidate of modifier K on schedule S
//   rule RAYS                      effective_cfg, the candidate it maps to and that candidate's row
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../gpu-ray-tracing_amd/csrc/tune.hpp"

using mrt::TuneState;

namespace {

struct InFlight {
    int slot;
    float ms;
    long ready;   // the key's launch index from which the timing is readable
};
struct Key {
    long clock = 0;   // launches of this key
    std::vector<InFlight> inFlight;
    int seen[4] = {-2, -2, -2, -2};   // stage1, stage1b, stage2, locked at the last state line
};

double base[TuneState::kSchedules], modf_[TuneState::kStage2];
std::map<std::pair<int, int>, double> pairs;
long lag = 0;   // < 0: never
int bvhMb = 0, cus = 256, xcds = 8, wantRule = -1;
uint32_t flags = 0;
mrt_launch_cfg user;
mrt::TuneTable table;
std::map<TuneState*, Key> keys;

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "tune_driver: %s\n", what.c_str());
    std::exit(2);
}

void parse_list(const char* s, double* out, int n) {
    for (int i = 0; i < n; i++) {
        char* end = nullptr;
        out[i] = std::strtod(s, &end);
        if (end == s || (i + 1 < n ? *end != ',' : *end != 0)) die("expected " + std::to_string(n) + " comma-separated numbers");
        s = end + 1;
    }
}

void print_cfg(const char* tag, const mrt_launch_cfg& c) {
    std::printf("%s waves=%d threshold=%d queues=%d lds=%d groups=%d wide=%d slack=%d rounds=%d tail=%d shared=%d "
                "block=%d sort=%d mask=%d\n",
                tag, c.waves_per_cu, c.fetch_threshold, c.num_queues, c.lds_stack, c.lane_groups, c.wide, c.spec_slack,
                c.static_rounds, c.tail_lanes, c.queue_shared, c.queue_block, c.ray_sort, c.queue_xcc_mask);
}

int32_t* cfg_field(const std::string& f) {
    const struct { const char* name; int32_t* p; } fields[] = {
        {"waves_per_cu", &user.waves_per_cu}, {"fetch_threshold", &user.fetch_threshold}, {"num_queues", &user.num_queues},
        {"lane_groups", &user.lane_groups},   {"spec_slack", &user.spec_slack},           {"autotune", &user.autotune},
        {"tail_lanes", &user.tail_lanes}};
    for (const auto& x : fields)
        if (f == x.name) return x.p;
    die("unknown cfg field " + f);
}

void launch(int rays, int variant, const void* stream) {
    const mrt_launch_cfg rule = mrt::effective_cfg(user, cus, (int64_t)bvhMb << 20, rays);
    if (wantRule >= 0 && mrt::rule_candidate(rule) != wantRule) die("the rule of this batch is not --rule");
    TuneState* st = table.lookup(user, rule, flags, rays, variant, stream);
    if (!st) {
        std::printf("launch cand=-1 info=-1 locked=0\n");
        return;
    }
    Key& k = keys[st];
    for (size_t i = 0; i < k.inFlight.size();) {
        if (lag < 0 || k.inFlight[i].ready > k.clock) {
            i++;
            continue;
        }
        st->slot_done(k.inFlight[i].slot, k.inFlight[i].ms);
        k.inFlight.erase(k.inFlight.begin() + (long)i);
    }
    int slot = -1;
    const int cand = st->next_launch(&slot);
    if (slot < -1 || slot >= TuneState::kSlots) die("slot out of range");
    const int now[4] = {st->stage1, st->stage1b, st->stage2, st->locked};
    if (std::memcmp(now, k.seen, sizeof(now)) != 0) {
        std::memcpy(k.seen, now, sizeof(now));
        std::printf("state stage1=%d stage1b=%d stage2=%d s3mod=%d s3sched=%d,%d,%d,%d,%d,%d locked=%d inherited=%d\n",
                    st->stage1, st->stage1b, st->stage2, st->s3mod, st->s3sched[0], st->s3sched[1], st->s3sched[2],
                    st->s3sched[3], st->s3sched[4], st->s3sched[5], st->locked, (int)st->inherited);
    }
    int sched = cand, mod = -1;
    st->decode(cand, &sched, &mod);
    const mrt_launch_cfg cfg = mrt::tune_candidate(xcds, rule, cand, st);
    if (slot >= 0) {
        const auto p = pairs.find({sched, mod});
        const double f = p != pairs.end() ? p->second : (mod >= 0 ? modf_[mod] : 1.0);
        k.inFlight.push_back({slot, (float)(base[sched] * f), k.clock + 1 + lag});
        st->slot_started(slot, cand);
    }
    k.clock++;
    std::printf("launch cand=%d info=0x%x locked=%d slot=%d explored=%d sched=%d mod=%d waves=%d queues=%d\n", cand,
                st->info_code(cand), st->locked >= 0 ? 1 : 0, slot, st->launches, sched, mod, cfg.waves_per_cu, cfg.num_queues);
}

}  // namespace

int main(int argc, char** argv) {
    for (double& b : base) b = 1.0;
    for (double& m : modf_) m = 1.0;
    // the library's defaults (launch_plan.cpp default_cfg) in the fields the tuner reads
    user = mrt_launch_cfg{};
    user.num_queues = -1;
    user.lds_stack = 16;
    user.lane_groups = 1;
    user.wide = 1;
    user.spec_slack = mrt::kDefaultSpecSlack;
    user.static_rounds = 1;
    user.autotune = 1;
    user.tail_lanes = mrt::kDefaultTailLanes;

    int i = 1;
    auto arg = [&]() -> const char* {
        if (i >= argc) die("missing argument");
        return argv[i++];
    };
    auto num = [&]() { return (int)std::strtol(arg(), nullptr, 0); };
    while (i < argc) {
        const std::string op = arg();
        if (op == "--base") parse_list(arg(), base, TuneState::kSchedules);
        else if (op == "--mod") parse_list(arg(), modf_, TuneState::kStage2);
        else if (op == "--pair") {
            int s = 0, k = 0;
            double f = 0;
            if (std::sscanf(arg(), "%d:%d:%lf", &s, &k, &f) != 3) die("--pair S:K:F");
            pairs[{s, k}] = f;
        } else if (op == "--lag") {
            const std::string v = arg();
            lag = v == "never" ? -1 : std::strtol(v.c_str(), nullptr, 0);
        } else if (op == "--bvh-mb") bvhMb = num();
        else if (op == "--cus") cus = num();
        else if (op == "--xcds") xcds = num();
        else if (op == "--rule") wantRule = num();
        else if (op == "cfg") {
            int32_t* f = cfg_field(arg());
            *f = num();
        } else if (op == "flags") flags = (uint32_t)num();
        else if (op == "launch") {
            const int rays = num(), variant = num();
            const void* stream = reinterpret_cast<const void*>((intptr_t)num());
            int n = 1;
            if (i < argc && argv[i][0] >= '0' && argv[i][0] <= '9') n = num();
            for (int j = 0; j < n; j++) launch(rays, variant, stream);
        } else if (op == "import") {
            std::vector<mrt_tuned_schedule> in((size_t)num());
            for (auto& e : in) {
                e.num_rays = num();
                e.variant = num();
                e.candidate = num();
                e.version = num();
            }
            const int rc = table.import_schedules(in.data(), (int)in.size());
            std::printf("import rc=%d keys=%d\n", rc, (int)table.tunes.size());
        } else if (op == "export") {
            mrt_tuned_schedule out[128];
            const int n = table.export_schedules(out, 128);
            std::printf("export n=%d\n", n);
            for (int j = 0; j < n && j < 128; j++)
                std::printf("exported rays=%d variant=%d candidate=%d version=%d\n", out[j].num_rays, out[j].variant,
                            out[j].candidate, out[j].version);
        } else if (op == "schedules") {
            for (int c = 0; c < TuneState::kSchedules; c++)
                print_cfg(("schedule " + std::to_string(c) + " strided_waves=" + std::to_string(mrt::kStridedWaves)).c_str(),
                          mrt::tune_candidate(xcds, user, c, nullptr));
        } else if (op == "modifier") {
            TuneState st;
            st.stage1 = num();
            print_cfg("modifier", mrt::tune_candidate(xcds, user, TuneState::kSchedules + num(), &st));
        } else if (op == "rule") {
            const mrt_launch_cfg rule = mrt::effective_cfg(user, cus, (int64_t)bvhMb << 20, num());
            std::printf("rule index=%d\n", mrt::rule_candidate(rule));
            print_cfg("rule", rule);
            print_cfg("row ", mrt::tune_candidate(xcds, rule, mrt::rule_candidate(rule), nullptr));
        } else die("unknown op " + op);
    }
    table.clear();
    return 0;
}
