// refit_plan.cpp — the height levels of a Compact2 tree (refit_plan.hpp). The
// other half of a refit plan, the wide-child source map, comes out of the collapse
// itself (build_wide4's srcMap, wide_bvh.cpp): after a refit the surface areas
// differ, so collapsing the refitted nodes again would choose other children.
#include "refit_plan.hpp"

namespace mrt {

const char* refit_levels(const int32_t* nodes, int64_t numNodes, RefitLevels* out) {
    out->order.clear();
    out->offsets.clear();
    if (!nodes || numNodes < 1) return "no nodes";
    if (numNodes > ((int64_t)1 << 26)) return "more than 2^26 nodes";   // 4 GiB of records: the bind limit

    // Parents before children from node 0, every ref checked.
    std::vector<int32_t> pre;
    pre.reserve((size_t)numNodes);
    std::vector<int32_t> height((size_t)numNodes, -1);   // -1 = not reached yet
    std::vector<int32_t> stack{0};
    height[0] = 0;
    while (!stack.empty()) {
        const int32_t n = stack.back();
        stack.pop_back();
        pre.push_back(n);
        for (int i = 0; i < 2; i++) {
            const int32_t ref = nodes[(int64_t)n * 16 + 12 + i];
            if (ref < 0) continue;   // a leaf
            if (ref % 4 != 0 || ref / 4 >= numNodes) return "a child ref points outside the node array";
            if (height[(size_t)(ref / 4)] >= 0) return "a node record is reached twice (not a tree)";
            height[(size_t)(ref / 4)] = 0;
            stack.push_back(ref / 4);
        }
    }
    if ((int64_t)pre.size() != numNodes) return "a node record is not reachable from node 0";

    // Heights, children first (the reverse of a parent-first order).
    int32_t top = 0;
    for (size_t k = pre.size(); k-- > 0;) {
        const int32_t n = pre[k];
        int32_t h = 0;
        for (int i = 0; i < 2; i++) {
            const int32_t ref = nodes[(int64_t)n * 16 + 12 + i];
            if (ref >= 0 && height[(size_t)(ref / 4)] + 1 > h) h = height[(size_t)(ref / 4)] + 1;
        }
        height[(size_t)n] = h;
        if (h > top) top = h;
    }

    // Counting sort by height, ascending node index inside a level.
    out->offsets.assign((size_t)top + 2, 0);
    for (int64_t n = 0; n < numNodes; n++) out->offsets[(size_t)height[(size_t)n] + 1]++;
    for (size_t h = 1; h < out->offsets.size(); h++) out->offsets[h] += out->offsets[h - 1];
    out->order.resize((size_t)numNodes);
    std::vector<int64_t> next(out->offsets.begin(), out->offsets.end() - 1);
    for (int64_t n = 0; n < numNodes; n++) out->order[(size_t)next[(size_t)height[(size_t)n]]++] = (int32_t)n;
    return nullptr;
}

}  // namespace mrt
