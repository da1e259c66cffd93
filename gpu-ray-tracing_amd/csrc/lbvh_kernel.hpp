// lbvh_kernel.hpp — launch interface between the C-ABI glue (build_api.cpp) and the
// gfx950 kernels that build a linear BVH's topology into Compact2 buffers
// (lbvh_kernel.hip). Boxes and Woop rows are the refit kernels' (refit_kernel.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mrt {

// One build's inputs, outputs and scratch (all device pointers).
struct LbvhBuild {
    const float* vertices;       // 3 per vertex
    int64_t numVertices;
    const int32_t* triangles;    // 3 vertex indices per triangle
    int numTriangles;            // 1 .. lbvh::kMaxTriangles
    int maxLeaf;                 // 1 .. 8
    // Outputs, sized by lbvh::max_records / max_slots.
    uint32_t* nodes;
    uint32_t* woop;
    int32_t* triIndex;
    // Scratch (lbvh_carve).
    float* partial;              // 6 per block of the bounds launch
    float* bounds;               // lo.xyz, hi.xyz of the centroids
    uint64_t* codes;             // per triangle, then sorted
    uint64_t* codesSorted;
    int32_t* ids;
    int32_t* idsSorted;
    int32_t* first;              // per Karras node: its range and split
    int32_t* last;
    int32_t* split;
    int32_t* kept;               // n entries: node k becomes a record (entry n - 1 stays 0)
    int32_t* leafStart;          // n + 1 entries: a leaf begins at sorted position p (entry n stays 0)
    int32_t* keptRank;           // exclusive sums; keptRank[n - 1] = records, leafRank[n] = leaves
    int32_t* leafRank;
    void* primTemp;              // the sort's and the scans' temporary storage
    size_t primTempBytes;
};

// Bytes of scratch a build of numTriangles needs (the sort's and scans' temporary storage
// included, asked of rocPRIM for the current device), and b's scratch pointers set into it.
hipError_t lbvh_scratch_bytes(int numTriangles, size_t* bytes, size_t* primTempBytes);
void lbvh_carve(LbvhBuild& b, void* scratch, size_t primTempBytes);

// Phase 1: centroid bounds, keys, the stable sort by key (values: triangle ids).
hipError_t launch_lbvh_sort(const LbvhBuild& b, hipStream_t s);
// Phase 2 (more than maxLeaf triangles): hierarchy, kept / leaf-start flags, their prefix
// sums, and the emission of records (child refs; boxes zero), zeroed Woop rows, triIndex
// and terminators.
hipError_t launch_lbvh_emit(const LbvhBuild& b, hipStream_t s);
// Phase 2 of at most maxLeaf triangles: one record, child 0 the leaf of all triangles,
// child 1 an empty leaf.
hipError_t launch_lbvh_emit_single(const LbvhBuild& b, hipStream_t s);
// After the boxes of a one-record tree: the empty leaf's box = child 0's box.
hipError_t launch_lbvh_empty_leaf_box(uint32_t* nodes, hipStream_t s);

}  // namespace mrt
