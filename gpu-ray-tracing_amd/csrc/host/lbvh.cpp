// lbvh.cpp — a linear BVH (Morton order, Karras 2012 hierarchy, leaves of at most
// maxLeaf triangles) built straight into Compact2 buffers: the CPU statement of the
// device build (csrc/lbvh_kernel.hip, mrt_tracer_build) and mrth_bvh_build_lbvh. No
// reference counterpart. Keys, order, hierarchy and numbering are lbvh_common.hpp's,
// the same code the kernels run; boxes and Woop rows are a refit of the emitted
// topology (refit.cpp), as on the device. Single-threaded: the bytes depend on nothing
// but the input.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../lbvh_common.hpp"
#include "bvh.hpp"

namespace mrt {

bool build_lbvh(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                int maxLeaf, Compact2& out, LbvhStats* stats, std::string* err) {
    auto fail = [&](const char* what) {
        if (err) *err = what;
        return false;
    };
    if (numTriangles < 1 || !triangles || numVertices < 0 || (numVertices && !vertices))
        return fail("lbvh: bad vertex / triangle arrays");
    if (maxLeaf < 1 || maxLeaf > lbvh::kMaxLeafLimit) return fail("lbvh: max_leaf_size outside 1..8");
    if (numTriangles > lbvh::kMaxTriangles) return fail("lbvh: too many triangles");
    const int n = (int)numTriangles;

    // Keys: the centroid bounds, then one code per triangle (0 for an out-of-range triangle).
    std::vector<float> centroid((size_t)n * 3);
    std::vector<char> inRange((size_t)n);
    lbvh::Bounds all = lbvh::bounds_empty();
    for (int i = 0; i < n; i++) {
        const int32_t* t = triangles + (size_t)i * 3;
        inRange[(size_t)i] = lbvh::tri_in_range(t, numVertices);
        if (!inRange[(size_t)i]) continue;
        float* c = &centroid[(size_t)i * 3];
        lbvh::tri_centroid(vertices + (size_t)t[0] * 3, vertices + (size_t)t[1] * 3, vertices + (size_t)t[2] * 3, c);
        lbvh::bounds_grow(all, c);
    }
    std::vector<uint64_t> code((size_t)n);
    for (int i = 0; i < n; i++) code[(size_t)i] = inRange[(size_t)i] ? lbvh::tri_code(&centroid[(size_t)i * 3], all) : 0;

    // Order: stable by code, so equal codes stay in index order.
    std::vector<int32_t> ids((size_t)n);
    std::iota(ids.begin(), ids.end(), 0);
    std::stable_sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) { return code[(size_t)a] < code[(size_t)b]; });
    std::vector<uint64_t> sorted((size_t)n);
    for (int p = 0; p < n; p++) sorted[(size_t)p] = code[(size_t)ids[(size_t)p]];

    const int64_t slotsBound = lbvh::max_slots(n);
    int64_t records = 0, leaves = 0;
    if (n <= maxLeaf) {
        // One record: child 0 the leaf of all triangles, child 1 an empty leaf (the wrapper
        // create_compact2 makes for a leaf root).
        records = 1;
        leaves = 2;
        out.nodes.assign(16, 0);
        out.woop.assign((size_t)(3 * n + 2) * 4, 0);
        out.triIndex.assign((size_t)(3 * n + 2), 0);
        for (int p = 0; p < n; p++) out.triIndex[(size_t)3 * p] = ids[(size_t)p];
        for (int s : {3 * n, 3 * n + 1})
            for (int k = 0; k < 4; k++) out.woop[(size_t)s * 4 + k] = (int32_t)woop::kTerminatorBits;
        out.nodes[12] = ~0;
        out.nodes[13] = ~(3 * n + 1);
    } else {
        // Hierarchy, flags and their exclusive sums.
        std::vector<lbvh::Node> node((size_t)n - 1);
        std::vector<int32_t> keptRank((size_t)n, 0), leafStart((size_t)n + 1, 0), leafRank((size_t)n + 1, 0);
        for (int k = 0; k < n - 1; k++) {
            const lbvh::Node nd = node[(size_t)k] = lbvh::karras_node(sorted.data(), n, k);
            keptRank[(size_t)k] = (int32_t)records;
            if (nd.last - nd.first + 1 <= maxLeaf) continue;
            records++;
            if (nd.split - nd.first + 1 <= maxLeaf) leafStart[(size_t)nd.first] = 1;
            if (nd.last - nd.split <= maxLeaf) leafStart[(size_t)nd.split + 1] = 1;
        }
        for (int p = 0; p <= n; p++) {
            leafRank[(size_t)p] = (int32_t)leaves;
            leaves += leafStart[(size_t)p];
        }
        const int64_t slots = 3 * (int64_t)n + leaves;
        if (slots > slotsBound) return fail("lbvh: more leaves than triangles");
        out.nodes.assign((size_t)records * 16, 0);
        out.woop.assign((size_t)slots * 4, 0);
        out.triIndex.assign((size_t)slots, 0);
        // Emission: records by Karras index, slots by sorted position.
        for (int k = 0; k < n - 1; k++) {
            const lbvh::Node& nd = node[(size_t)k];
            if (nd.last - nd.first + 1 <= maxLeaf) continue;
            const int from[2] = {nd.first, nd.split + 1}, to[2] = {nd.split, nd.last}, child[2] = {nd.split, nd.split + 1};
            int32_t* rec = &out.nodes[(size_t)keptRank[(size_t)k] * 16];
            for (int i = 0; i < 2; i++)
                rec[12 + i] = to[i] - from[i] + 1 > maxLeaf ? keptRank[(size_t)child[i]] * 4
                                                           : ~lbvh::leaf_slot(from[i], leafRank[(size_t)from[i]]);
        }
        for (int p = 0; p < n; p++) {
            const int rank = leafRank[(size_t)p] + leafStart[(size_t)p] - 1;
            const int slot = lbvh::leaf_slot(p, rank);
            out.triIndex[(size_t)slot] = ids[(size_t)p];
            if (p == n - 1 || leafStart[(size_t)p + 1])
                for (int k = 0; k < 4; k++) out.woop[(size_t)(slot + 3) * 4 + k] = (int32_t)woop::kTerminatorBits;
        }
    }

    // Boxes and rows: exactly what a refit of that topology gives. The host refit refuses
    // an out-of-range vertex index (the device build skips and counts such a triangle).
    if (!refit_compact2(out, vertices, numVertices, triangles, numTriangles, err)) return false;
    if (n <= maxLeaf)
        for (int k = 0; k < 3; k++)
            for (int e = 0; e < 2; e++) out.nodes[(size_t)woop::box_word(1, k) + e] = out.nodes[(size_t)woop::box_word(0, k) + e];
    if (stats) {
        stats->records = records;
        stats->leaves = leaves;
        stats->slots = (int64_t)out.triIndex.size();
    }
    return true;
}

}  // namespace mrt
