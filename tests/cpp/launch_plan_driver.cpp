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
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../gpu-ray-tracing_amd/csrc/launch_plan.hpp"

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
        } else {
            die("unknown op " + op);
        }
    }
    return 0;
}
