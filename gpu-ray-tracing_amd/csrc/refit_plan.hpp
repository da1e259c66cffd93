// refit_plan.hpp — what a device refit (refit_kernel.hip) needs besides the bound
// buffers, computed once per bound tree on the host (refit_plan.cpp: no HIP, like
// tune.cpp and wide_bvh.cpp's collapse).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mrt {

// The inner nodes of a Compact2 node array grouped by height: a node whose children
// are both leaves has height 0, any other 1 + the largest height of its inner
// children. order holds every node once, level h at [offsets[h], offsets[h + 1]),
// ascending inside a level. A node's inner children lie in strictly lower levels, so
// one launch per level (in rising order) sees every child box finished; the level
// sizes never grow with the height (each node of level h + 1 owns a child of level h).
struct RefitLevels {
    std::vector<int32_t> order;
    std::vector<int64_t> offsets;   // levels + 1 entries
    int levels() const { return (int)offsets.size() - 1; }
};

// Any valid tree, whatever its numbering (not only the serialiser's parent-before-child
// one). Null on success; else why the array is refused: a child ref outside the array
// or not a record's first float4, a record reached twice, or a record never reached
// from node 0 (a refit would leave its boxes stale).
const char* refit_levels(const int32_t* nodes, int64_t numNodes, RefitLevels* out);

}  // namespace mrt
