// scene_kernel.hpp — launch interface between the C-ABI glue (scene_api.cpp) and the gfx950
// kernels of scene_kernel.hip: a scene's per-triangle normals and colours from device vertices
// (mrt_scene_attributes), and the cost sums of a bound Compact2 tree (mrt_tracer_tree_cost).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/mrt.h"

namespace mrt {

// Lanes of a workgroup of either kernel: one per triangle, or one per child slot (two per record).
constexpr int kSceneBlock = 256;
// Lanes of the cost's final step (one wave): lane j adds the partials [j * c, (j + 1) * c) in
// index order, c = ceil(partials / kCostFinalLanes), then the wave adds its lanes.
constexpr int kCostFinalLanes = 64;

struct SceneAttrArgs {
    const float* vertices;        // 3 per vertex
    int64_t numVertices;
    const int32_t* triangles;     // 3 vertex indices per triangle
    int numTriangles;             // 1 .. scene::kMaxTriangles
    const float* triDiffuse;      // 4 per triangle, or null: the default material
    float* triNormals;            // 3 per triangle, or null
    uint32_t* triShadedColor;     // or null
    uint32_t* triMaterialColor;   // or null
    unsigned long long* skipped;  // or null: += triangles with a vertex index out of range
};

// One workgroup's sums, and the final sums before they become an mrt_tree_cost.
struct CostPartial {
    double inner, leaf, leafTri;
    long long leaves, triangles, skipped;
};

struct TreeCostArgs {
    const uint32_t* nodes;   // numNodes records of 16 words
    int numNodes;            // 1 .. 2^26
    const uint32_t* woop;    // woopSlots float4 slots
    int woopSlots;
    CostPartial* partials;   // cost_partials(numNodes) entries
    mrt_tree_cost* out;      // device
};

inline int cost_partials(int64_t numNodes) { return (int)((2 * numNodes + kSceneBlock - 1) / kSceneBlock); }

// One launch, one lane per triangle.
hipError_t launch_scene_attributes(const SceneAttrArgs& a, hipStream_t s);
// Two launches: one lane per child slot and a partial per workgroup, then the final step.
hipError_t launch_tree_cost(const TreeCostArgs& a, hipStream_t s);

}  // namespace mrt
