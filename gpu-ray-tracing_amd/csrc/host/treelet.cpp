// treelet.cpp — treelet restructuring of a Compact2 tree on the host (treelet.hpp; behind
// mrth_bvh_optimize): the CPU reference of mrt_tracer_optimize. Records of equal height have
// disjoint subtrees and a restructuring only permutes records inside its root's subtree, so the
// records of one level are independent, and a level's roots were written by no level below.
#include "treelet.hpp"

#include <cstddef>
#include <vector>

#include "../treelet_common.hpp"

using std::size_t;

namespace mrt {

namespace {

// The records by height, lowest first; mrt_refit_plan's levels (csrc/refit_plan.cpp).
const char* height_levels(const int32_t* nodes, int64_t numNodes, std::vector<int32_t>* order,
                          std::vector<int64_t>* offsets) {
    if (!nodes || numNodes < 1) return "no nodes";
    if (numNodes > ((int64_t)1 << 26)) return "more than 2^26 nodes";
    std::vector<int32_t> pre;
    pre.reserve((size_t)numNodes);
    std::vector<int32_t> height((size_t)numNodes, -1);
    std::vector<int32_t> stack{0};
    height[0] = 0;
    while (!stack.empty()) {
        const int32_t n = stack.back();
        stack.pop_back();
        pre.push_back(n);
        for (int i = 0; i < 2; i++) {
            const int32_t ref = nodes[(int64_t)n * 16 + 12 + i];
            if (ref < 0) continue;
            if (ref % 4 != 0 || ref / 4 >= numNodes) return "a child ref points outside the node array";
            if (height[(size_t)(ref / 4)] >= 0) return "a node record is reached twice (not a tree)";
            height[(size_t)(ref / 4)] = 0;
            stack.push_back(ref / 4);
        }
    }
    if ((int64_t)pre.size() != numNodes) return "a node record is not reachable from node 0";
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
    offsets->assign((size_t)top + 2, 0);
    for (int64_t n = 0; n < numNodes; n++) (*offsets)[(size_t)height[(size_t)n] + 1]++;
    for (size_t h = 1; h < offsets->size(); h++) (*offsets)[h] += (*offsets)[h - 1];
    order->resize((size_t)numNodes);
    std::vector<int64_t> next(offsets->begin(), offsets->end() - 1);
    for (int64_t n = 0; n < numNodes; n++) (*order)[(size_t)next[(size_t)height[(size_t)n]]++] = (int32_t)n;
    return nullptr;
}

}  // namespace

const char* optimize_nodes(int32_t* nodes, int64_t numNodes, int rounds, OptimizeStats* stats) {
    if (rounds < 1 || rounds > kOptimizeMaxRounds) return "rounds outside 1..8";
    std::vector<int32_t> order;
    std::vector<int64_t> offsets;
    OptimizeStats st;
    uint32_t* words = reinterpret_cast<uint32_t*>(nodes);
    for (int r = 0; r < rounds; r++) {
        if (const char* why = height_levels(nodes, numNodes, &order, &offsets)) return why;
        st.considered[r] = numNodes - offsets[1];
        for (int64_t i = offsets[1]; i < numNodes; i++)   // level by level: order is sorted by height
            st.rewritten[r] += treelet::restructure(words, numNodes, order[(size_t)i]) ? 1 : 0;
        st.rounds = r + 1;
    }
    if (const char* why = height_levels(nodes, numNodes, &order, &offsets)) return why;
    st.levels = (int32_t)offsets.size() - 1;
    if (stats) *stats = st;
    return nullptr;
}

}  // namespace mrt
