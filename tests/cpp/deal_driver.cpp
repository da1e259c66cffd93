// deal_driver.cpp — the one-shot deal (csrc/deal_common.hpp), its grid (csrc/launch_plan.cpp) and
// the saved-schedule bits that carry it (csrc/tune.cpp) on the CPU. Host compiler only: no HIP,
// no libmrt. tests/test_deal.py reads its output; the same file built with
// -fsanitize=address,undefined runs the same cases as a stand-alone program.
//
//   deal_driver deal N B GROUPS_LOG2 [CUS WAVES OCC ENTRIES CAP_BYTES]
//       plans the one-shot grid of N rays (2^B-ray blocks, B = 0: contiguous) on a device of CUS
//       compute units at WAVES waves per CU, enumerates every launched lane and prints one line:
//       oneshot= blocks= lanes= spill_ints= dealt= twice= past= missing= group_bad= ref_bad=
//         dealt      lanes that hold a ray
//         twice      rays dealt to more than one lane
//         past       lanes dealt an index >= N (must be none: such a lane reports N, "no ray")
//         missing    rays below N that no lane holds
//         group_bad  B > 0: rays whose group is not (ray >> B) % 8
//         ref_bad    B = 0: lanes whose ray differs from the first strided round of the persistent
//                    kernels on the same grid (restated below from trace_kernel.hip strided_ray)
//   deal_driver plan N B CUS WAVES OCC ENTRIES [CAP_BYTES]
//       the plan with and without cfg.oneshot: oneshot= blocks= backfill= per_cu= dyn= spill_ints=, twice
//   deal_driver code CANDIDATE
//       imports one saved schedule (786432 rays) and prints rc=, the exported code and the
//       configuration its launch gets: backfill= oneshot= deal_block= waves= info=
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gpu-ray-tracing_amd/csrc/deal_common.hpp"
#include "../../gpu-ray-tracing_amd/csrc/launch_plan.hpp"
#include "../../gpu-ray-tracing_amd/csrc/tune.hpp"

namespace {

constexpr int kBlockThreads = 256;

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "deal_driver: %s\n", what.c_str());
    std::exit(2);
}

long long num(const char* s) {
    char* end = nullptr;
    const long long v = std::strtoll(s, &end, 0);
    if (end == s || *end) die(std::string("not a number: ") + s);
    return v;
}

// The first strided round of the persistent kernels (trace_kernel.hip strided_ray, roundBase 0,
// numQueues 0, no ray sort) for a lane of a grid of gridBlocks workgroups; n: no ray.
int strided_first_round(int n, int gridBlocks, int laneGroupsLog2, int block, int thread) {
    const int wavesTotal = gridBlocks * (kBlockThreads / 64);
    const int groups = (gridBlocks & 7) == 0 ? 8 : 1;
    const int group = block % groups;
    const int groupLanes = wavesTotal / groups * 64;
    const int blocksPerGroup = gridBlocks / groups;
    const int lane = thread & 63;
    const int localLane = ((thread >> 6) * blocksPerGroup + block / groups) * 64 + lane;
    const int left = n;
    if (left <= 0) return n;
    const int c = std::min(groupLanes, ((left + groups - 1) / groups + 63) & ~63);
    int chunkLane = localLane;
    if (laneGroupsLog2 > 0) {
        const int gl = 6 - laneGroupsLog2;
        const int w = localLane >> 6, sg = lane >> gl, p = lane & ((1 << gl) - 1);
        chunkLane = ((sg * (c >> 6) + w) << gl) + p;
    }
    return localLane < c ? std::min(group * c + chunkLane, n) : n;
}

mrt::LaunchPlanIn plan_in(int n, int b, int oneshot, char** rest, int nrest) {
    mrt::LaunchPlanIn in;
    in.numRays = n;
    in.backfill = 1;
    in.oneshot = oneshot;
    in.dealBlockLog2 = b;
    in.numCUs = nrest > 0 ? (int)num(rest[0]) : 1;
    in.wavesPerCU = nrest > 1 ? (int)num(rest[1]) : 4;
    in.occBlocks = nrest > 2 ? (int)num(rest[2]) : 1;
    in.spillEntries = nrest > 3 ? (int)num(rest[3]) : 48;
    if (nrest > 4) in.spillCapBytes = num(rest[4]);
    in.blockThreads = kBlockThreads;
    in.staticLds = 8192;
    in.ldsPerCU = 160 << 10;
    return in;
}

void print_plan(const mrt::LaunchPlan& p) {
    std::printf("plan oneshot=%d deal_block=%d blocks=%d backfill=%d per_cu=%d dyn=%d spill_ints=%lld\n", p.oneshot,
                p.dealBlockLog2, p.blocks, p.backfill, p.blocksPerCU, p.dynLds, (long long)p.spillInts);
}

int cmd_deal(int argc, char** argv) {
    if (argc < 3) die("deal N B GROUPS_LOG2 [CUS WAVES OCC ENTRIES CAP_BYTES]");
    const int n = (int)num(argv[0]), b = (int)num(argv[1]), lg = (int)num(argv[2]);
    const mrt::LaunchPlanIn in = plan_in(n, b, 1, argv + 3, argc - 3);
    const mrt::LaunchPlan p = mrt::plan_launch(in);
    long long dealt = 0, twice = 0, past = 0, missing = 0, groupBad = 0, refBad = 0;
    const long long lanes = (long long)p.blocks * kBlockThreads;
    if (p.oneshot) {
        std::vector<unsigned char> seen((size_t)n, 0);
        const int blocksPerGroup = p.blocks / mrt::deal::kGroups;
        for (int block = 0; block < p.blocks; block++)
            for (int t = 0; t < kBlockThreads; t++) {
                const int r = mrt::deal::lane_ray(n, b, lg, blocksPerGroup, block, t >> 6, t & 63);
                if (b == 0 && r != strided_first_round(n, p.blocks, lg, block, t)) refBad++;
                if (r == n) continue;
                if (r < 0 || r > n) {
                    past++;
                    continue;
                }
                dealt++;
                if (seen[(size_t)r]++) twice++;
                if (b > 0 && ((r >> b) % mrt::deal::kGroups) != block % mrt::deal::kGroups) groupBad++;
            }
        for (int r = 0; r < n; r++) missing += seen[(size_t)r] == 0;
    }
    std::printf("deal oneshot=%d blocks=%d lanes=%lld spill_ints=%lld dealt=%lld twice=%lld past=%lld missing=%lld "
                "group_bad=%lld ref_bad=%lld\n",
                p.oneshot, p.blocks, lanes, (long long)p.spillInts, dealt, twice, past, missing, groupBad, refBad);
    return 0;
}

int cmd_plan(int argc, char** argv) {
    if (argc < 6) die("plan N B CUS WAVES OCC ENTRIES [CAP_BYTES]");
    const int n = (int)num(argv[0]), b = (int)num(argv[1]);
    print_plan(mrt::plan_launch(plan_in(n, b, 1, argv + 2, argc - 2)));
    print_plan(mrt::plan_launch(plan_in(n, b, 0, argv + 2, argc - 2)));
    return 0;
}

int cmd_code(int argc, char** argv) {
    if (argc < 1) die("code CANDIDATE");
    const int rays = 786432, variant = 342;
    mrt::TuneTable table;
    const mrt_tuned_schedule e{rays, variant, (int32_t)num(argv[0]), MRT_TUNE_VERSION};
    const int rc = table.import_schedules(&e, 1);
    std::printf("code rc=%d keys=%d", rc, (int)table.tunes.size());
    if (rc == 0) {
        mrt_tuned_schedule out{};
        table.export_schedules(&out, 1);
        mrt_launch_cfg user{};
        user.autotune = 1;
        user.num_queues = -1;
        user.lane_groups = 1;
        user.spec_slack = mrt::kDefaultSpecSlack;
        user.tail_lanes = mrt::kDefaultTailLanes;
        user.lds_stack = 16;
        user.wide = 1;
        user.static_rounds = 1;
        mrt::TuneState* st = table.lookup(user, user, 0, rays, variant, nullptr);
        if (!st) die("an imported key was not found");
        int slot = -1;
        const int cand = st->next_launch(&slot);
        const mrt_launch_cfg cfg = mrt::tune_candidate(8, user, cand, st);
        std::printf(" exported=%d backfill=%d oneshot=%d deal_block=%d waves=%d groups=%d slack=%d info=%d", out.candidate,
                    cfg.backfill, cfg.oneshot, cfg.deal_block, cfg.waves_per_cu, cfg.lane_groups, cfg.spec_slack,
                    st->info_code(cand));
    }
    std::printf("\n");
    table.clear();
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) die("usage: deal_driver deal|plan|code ...");
    const std::string op = argv[1];
    if (op == "deal") return cmd_deal(argc - 2, argv + 2);
    if (op == "plan") return cmd_plan(argc - 2, argv + 2);
    if (op == "code") return cmd_code(argc - 2, argv + 2);
    die("unknown operation " + op);
}
