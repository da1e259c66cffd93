// path_plan.cpp — the path frame's plan (path_plan.hpp). The order of the checks is the order
// include/mrt.h documents: shape (MRT_ERR_INVALID_ARG), limits (MRT_ERR_TOO_LARGE), then empty.
#include "path_plan.hpp"

#include "../../include/mrt.h"
#include "path_limits.hpp"

namespace mrt {
namespace {

PathPlan refuse(int rc, const char* why) { return PathPlan{rc, why, false, 0, 0, 0}; }

int grid_of(int64_t n) { return (int)((n + path::kThreads - 1) / path::kThreads); }

}  // namespace

PathPlan plan_path_extend(int32_t vertex, int32_t depth, int32_t numSamples, int32_t numSlots, int32_t numPaths) {
    if (numSlots < 0 || numPaths < 0 || numSamples < 1 || depth < 0 || vertex < 0 || vertex > depth)
        return refuse(MRT_ERR_INVALID_ARG, "path extend: bad vertex, depth, sample or slot count");
    if (depth > path::kMaxDepth) return refuse(MRT_ERR_TOO_LARGE, "path extend: depth above 64");
    if (numSlots > path::kMaxPaths || numPaths > path::kMaxPaths)
        return refuse(MRT_ERR_TOO_LARGE, "path extend: more paths than one call takes");
    if (vertex == 0 && numPaths < numSlots)
        return refuse(MRT_ERR_INVALID_ARG, "path extend: fewer radiance entries than paths started");
    PathPlan p{MRT_OK, "", numSlots == 0, grid_of(numSlots), 0, 0};
    p.scanRounds = (p.grid + path::kScanThreads - 1) / path::kScanThreads;
    p.scratchBytes = (size_t)p.grid * sizeof(int32_t);
    return p;
}

PathPlan plan_path_accumulate(int32_t numSlots, int32_t numPaths) {
    if (numSlots < 0 || numPaths < 0) return refuse(MRT_ERR_INVALID_ARG, "path accumulate: negative count");
    if (numSlots > path::kMaxPaths || numPaths > path::kMaxPaths)
        return refuse(MRT_ERR_TOO_LARGE, "path accumulate: more paths than one call takes");
    return PathPlan{MRT_OK, "", numSlots == 0, grid_of(numSlots), 0, 0};
}

PathPlan plan_path_resolve(int32_t numSamples, int32_t firstPrimary, int32_t numPrimary) {
    if (numSamples < 1 || firstPrimary < 0 || numPrimary < 0)
        return refuse(MRT_ERR_INVALID_ARG, "path resolve: bad batch shape");
    if ((int64_t)numPrimary * numSamples > path::kMaxPaths || (int64_t)firstPrimary + numPrimary > INT32_MAX)
        return refuse(MRT_ERR_TOO_LARGE, "path resolve: more paths than one call takes");
    return PathPlan{MRT_OK, "", numPrimary == 0, grid_of(numPrimary), 0, 0};
}

}  // namespace mrt
