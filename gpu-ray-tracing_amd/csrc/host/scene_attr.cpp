// scene_attr.cpp — a scene's per-triangle normals and colours and a Compact2 tree's cost sums on
// the CPU: the statements mrt_scene_attributes and mrt_tracer_tree_cost (csrc/scene_kernel.hip)
// are checked against, term for term (csrc/scene_common.hpp).
#include "scene_attr.hpp"

#include <cstring>

#include "../scene_common.hpp"
#include "host_error.hpp"

namespace mrt {

int64_t scene_attributes(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                         const float* triDiffuse, float* triNormals, uint32_t* triShadedColor,
                         uint32_t* triMaterialColor) {
    float light[3], defaultDiffuse[4];
    scene::light_dir(light);
    scene::default_diffuse(defaultDiffuse);
    int64_t skipped = 0;
    for (int64_t i = 0; i < numTriangles; i++) {
        const int32_t* t = triangles + 3 * i;
        float n[3] = {0.0f, 0.0f, 0.0f};
        const uint64_t nv = (uint64_t)numVertices;
        if ((uint64_t)(int64_t)t[0] >= nv || (uint64_t)(int64_t)t[1] >= nv || (uint64_t)(int64_t)t[2] >= nv)
            skipped++;
        else
            scene::tri_normal(vertices + 3 * (int64_t)t[0], vertices + 3 * (int64_t)t[1], vertices + 3 * (int64_t)t[2], n);
        const float* diffuse = triDiffuse ? triDiffuse + 4 * i : defaultDiffuse;
        if (triNormals) std::memcpy(triNormals + 3 * i, n, 12);
        if (triMaterialColor) triMaterialColor[i] = scene::to_abgr(diffuse);
        if (triShadedColor) triShadedColor[i] = scene::shade(n, light, diffuse);
    }
    return skipped;
}

namespace {
woop::Box slot_box(const int32_t* rec, int side) {
    woop::Box b;
    for (int k = 0; k < 3; k++) {
        const int w = woop::box_word(side, k);
        std::memcpy(&b.lo[k], rec + w, 4);
        std::memcpy(&b.hi[k], rec + w + 1, 4);
    }
    return b;
}
}  // namespace

void tree_cost(const int32_t* nodes, int64_t numNodes, const int32_t* woop, int64_t woopSlots, mrth_tree_cost* out) {
    mrth_tree_cost c{};
    c.records = numNodes;
    for (int64_t n = 0; n < numNodes; n++) {
        const int32_t* rec = nodes + 16 * n;
        for (int side = 0; side < 2; side++) {
            const int32_t ref = rec[12 + side];
            double area;
            const bool ok = scene::tree_cost_term(slot_box(rec, side), &area);
            if (!ok) c.skipped++;
            if (ref >= 0) {
                if (ok) c.inner_area += area;
                continue;
            }
            const int64_t count =
                scene::leaf_triangles(ref, woopSlots, [woop](int64_t s) { return (uint32_t)woop[s * 4]; });
            c.leaves++;
            c.triangles += count;
            if (ok) {
                c.leaf_area += area;
                c.leaf_tri_area += area * (double)count;
            }
        }
    }
    if (numNodes > 0) {
        double root;
        if (scene::tree_cost_term(woop::box_union(slot_box(nodes, 0), slot_box(nodes, 1)), &root)) {
            c.root_area = root;
            c.inner_area += root;
        } else {
            c.skipped++;
        }
    }
    *out = c;
}

}  // namespace mrt

extern "C" {

int mrth_scene_attributes(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                          const float* triDiffuse, float* triNormals, uint32_t* triShadedColor,
                          uint32_t* triMaterialColor, int64_t* skipped) {
    if (numVertices < 0 || numTriangles < 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "scene_attributes: negative count");
    if (!triNormals && !triShadedColor && !triMaterialColor)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "scene_attributes: no output");
    if (numTriangles == 0) return MRTH_OK;
    if (!vertices || !triangles)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "scene_attributes: null vertices or triangles");
    if (numTriangles > mrt::scene::kMaxTriangles)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "scene_attributes: more than 67108863 triangles");
    const int64_t n = mrt::scene_attributes(vertices, numVertices, triangles, numTriangles, triDiffuse, triNormals,
                                            triShadedColor, triMaterialColor);
    if (skipped) *skipped += n;
    return MRTH_OK;
}

}  // extern "C"
