// refit_kernel.hpp — launch interface between the C-ABI glue (refit_api.cpp: enqueue_refit, which
// the device build of build_api.cpp runs too) and the gfx950 refit kernels (refit_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mrt {

// A refit's buffers. nodes / woop are the bound Compact2 buffers, written in place.
struct RefitArgs {
    uint32_t* nodes;             // numNodes records of 16 words
    int numNodes;                // <= 2^26
    uint32_t* woop;              // woopSlots float4 slots
    int woopSlots;               // < 2^28
    const int32_t* triIndex;     // one per slot
    const float* vertices;       // 3 per vertex
    int64_t numVertices;
    const int32_t* triangles;    // 3 vertex indices per triangle
    int64_t numTriangles;
    uint8_t* valid;              // 2 per node: child i holds a triangle somewhere below it (this refit)
    unsigned long long* skipped; // += leaf triangles left out for an out-of-range triIndex / vertex index
};

// Levels of at most this many nodes are walked by one workgroup (launch_refit_tail).
constexpr int kRefitTailNodes = 1024;

// One thread per (node, leaf child): Woop rows, the leaf's box into its parent's slot.
hipError_t launch_refit_leaves(const RefitArgs& a, hipStream_t s);
// One thread per node of order[begin, begin + count): the boxes of its inner children.
hipError_t launch_refit_level(const RefitArgs& a, const int32_t* order, int begin, int count, hipStream_t s);
// Levels [firstLevel, numLevels) in one workgroup, a barrier between levels; offsets:
// device int32[numLevels + 1] into order.
hipError_t launch_refit_tail(const RefitArgs& a, const int32_t* order, const int32_t* offsets, int firstLevel,
                             int numLevels, hipStream_t s);
// One thread per wide child: the six planes of Compact2 slot wideSrc[4 * node + child]
// into the exact 4-wide array (128 B per node); absent children (-1) are left alone.
hipError_t launch_refit_wide(const RefitArgs& a, const int32_t* wideSrc, uint32_t* wideNodes, int numWide,
                             hipStream_t s);

}  // namespace mrt
