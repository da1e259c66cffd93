// path_plan.hpp — what the path frame's C-ABI (path_api.cpp) decides before it launches anything:
// the scalar checks and limits of a call, its grid, the scan's rounds and the count scratch. Plain
// C++ with no HIP in it (the host compiler builds path_plan.cpp), so tests/cpp/path_driver.cpp runs
// it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mrt {

struct PathPlan {
    int rc;            // MRT_OK, or the error the call returns before it touches anything
    const char* why;
    bool empty;        // a count of zero: MRT_OK, nothing launched
    int grid;          // workgroups of path::kThreads lanes: one lane per slot (resolve: per primary)
    int scanRounds;    // extend only: rounds of the one scan workgroup over the grid's counts
    size_t scratchBytes;   // extend only: the counts
};

PathPlan plan_path_extend(int32_t vertex, int32_t depth, int32_t numSamples, int32_t numSlots, int32_t numPaths);
PathPlan plan_path_accumulate(int32_t numSlots, int32_t numPaths);
PathPlan plan_path_resolve(int32_t numSamples, int32_t firstPrimary, int32_t numPrimary);

}  // namespace mrt
