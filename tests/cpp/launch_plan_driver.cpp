// launch_plan_driver.cpp — runs the launch plan (csrc/launch_plan.cpp) on the CPU: the grid, the
// residency cap and the spill slab mrt_api.cpp would launch with, from figures given on the
// command line in place of a device's. Built from this file and launch_plan.cpp alone by the
// host compiler: no HIP, no libmrt. tests/test_launch_plan.py reads its output.
//
//   launch_plan_driver OP...
//
//   plan RAYS K CUS WAVES STATIC_LDS LDS_PER_CU OCC SPILL_ENTRIES [SPILL_CAP_BYTES]
//        one line: blocks, backfill (the effective k, 0 = persistent), per_cu, dyn, spill_ints
//   dyn BLOCKS STATIC_LDS LDS_PER_CU
//        cap_dyn_lds: the dynamic LDS bytes that admit exactly BLOCKS workgroups per CU, or -1
//   cfg [FIELD=VALUE]...
//        what mrt_tracer_set_config does with the library's default configuration with the listed
//        fields set: rc (0 accepted, 1 = MRT_ERR_INVALID_ARG) and every field after the sentinels
//        were resolved
//   waves CUS RAYS NUM_QUEUES WAVES_PER_CU
//        grid_waves_per_cu of the default configuration with these two fields
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../gpu-ray-tracing_amd/csrc/launch_plan.hpp"

namespace {
struct CfgField {
    const char* name;
    int32_t mrt_launch_cfg::*member;
};
const CfgField kCfgFields[] = {
    {"waves_per_cu", &mrt_launch_cfg::waves_per_cu},   {"fetch_threshold", &mrt_launch_cfg::fetch_threshold},
    {"num_queues", &mrt_launch_cfg::num_queues},       {"lds_stack", &mrt_launch_cfg::lds_stack},
    {"lane_groups", &mrt_launch_cfg::lane_groups},     {"wide", &mrt_launch_cfg::wide},
    {"spec_slack", &mrt_launch_cfg::spec_slack},       {"static_rounds", &mrt_launch_cfg::static_rounds},
    {"autotune", &mrt_launch_cfg::autotune},           {"tail_lanes", &mrt_launch_cfg::tail_lanes},
    {"queue_shared", &mrt_launch_cfg::queue_shared},   {"queue_block", &mrt_launch_cfg::queue_block},
    {"ray_sort", &mrt_launch_cfg::ray_sort},           {"queue_xcc_mask", &mrt_launch_cfg::queue_xcc_mask},
    {"backfill", &mrt_launch_cfg::backfill},           {"oneshot", &mrt_launch_cfg::oneshot},
    {"deal_block", &mrt_launch_cfg::deal_block},
};
static_assert(sizeof(kCfgFields) / sizeof(kCfgFields[0]) * sizeof(int32_t) == sizeof(mrt_launch_cfg),
              "every field of mrt_launch_cfg is listed");
}  // namespace

int main(int argc, char** argv) {
    int i = 1;
    auto die = [](const std::string& what) {
        std::fprintf(stderr, "launch_plan_driver: %s\n", what.c_str());
        std::exit(2);
    };
    auto num = [&]() -> long long {
        if (i >= argc) die("missing argument");
        char* end = nullptr;
        const long long v = std::strtoll(argv[i], &end, 0);
        if (end == argv[i] || *end != 0) die(std::string("not a number: ") + argv[i]);
        i++;
        return v;
    };
    while (i < argc) {
        const std::string op = argv[i++];
        if (op == "plan") {
            mrt::LaunchPlanIn in;
            in.numRays = (int)num();
            in.backfill = (int)num();
            in.numCUs = (int)num();
            in.wavesPerCU = (int)num();
            in.staticLds = (int)num();
            in.ldsPerCU = (int)num();
            in.occBlocks = (int)num();
            in.spillEntries = (int)num();
            if (i < argc && argv[i][0] >= '0' && argv[i][0] <= '9') in.spillCapBytes = num();
            const mrt::LaunchPlan p = mrt::plan_launch(in);
            std::printf("plan blocks=%d backfill=%d per_cu=%d dyn=%d spill_ints=%lld\n", p.blocks, p.backfill, p.blocksPerCU,
                        p.dynLds, (long long)p.spillInts);
        } else if (op == "dyn") {
            const int blocks = (int)num(), staticLds = (int)num(), ldsPerCU = (int)num();
            std::printf("dyn %d\n", mrt::cap_dyn_lds(blocks, staticLds, ldsPerCU));
        } else if (op == "cfg") {
            mrt_launch_cfg user = mrt::default_cfg();
            for (const char* eq; i < argc && (eq = std::strchr(argv[i], '=')) != nullptr; i++) {
                const std::string name(argv[i], (size_t)(eq - argv[i]));
                const CfgField* field = nullptr;
                for (const CfgField& f : kCfgFields)
                    if (name == f.name) field = &f;
                if (!field) die("unknown field " + name);
                char* end = nullptr;
                user.*field->member = (int32_t)std::strtol(eq + 1, &end, 0);
                if (end == eq + 1 || *end != 0) die(std::string("not a number: ") + argv[i]);
            }
            const mrt_launch_cfg c = mrt::resolve_cfg(user);
            std::printf("cfg rc=%d", mrt::valid_cfg(c) ? 0 : 1);
            for (const CfgField& f : kCfgFields) std::printf(" %s=%d", f.name, (int)(c.*f.member));
            std::printf("\n");
        } else if (op == "waves") {
            const int cus = (int)num(), rays = (int)num();
            mrt_launch_cfg c = mrt::default_cfg();
            c.num_queues = (int)num();
            c.waves_per_cu = (int)num();
            std::printf("waves %d\n", mrt::grid_waves_per_cu(cus, c, rays));
        } else {
            die("unknown op " + op);
        }
    }
    return 0;
}
