// scene_attr.hpp — the CPU statements of mrt_scene_attributes and mrt_tracer_tree_cost over plain
// arrays (scene_attr.cpp; the arithmetic is csrc/scene_common.hpp's).
#pragma once
#include <cstdint>

#include "../../../include/mrt_host.h"

namespace mrt {

// Every triangle's normal and colours (null outputs are left out); returns the triangles with a
// vertex index outside [0, numVertices), which get the normal (0, 0, 0).
int64_t scene_attributes(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                         const float* triDiffuse, float* triNormals, uint32_t* triShadedColor,
                         uint32_t* triMaterialColor);

// The sums of numNodes Compact2 records, added in record order, side 0 before side 1.
void tree_cost(const int32_t* nodes, int64_t numNodes, const int32_t* woop, int64_t woopSlots, mrth_tree_cost* out);

}  // namespace mrt
