// treelet_kernel.hpp — launch interface between the C-ABI glue (optimize_api.cpp) and the gfx950
// treelet restructuring kernels (treelet_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mrt {

struct TreeletArgs {
    uint32_t* nodes;        // numNodes records of 16 words, rewritten in place
    int numNodes;           // <= 2^26
    unsigned* rewritten;    // += treelets whose records were rewritten
};

// Levels of at most this many records are walked by one workgroup (launch_treelet_tail): its
// 16 waves take 16 treelets at a time, so such a level costs at most four turns.
constexpr int kTreeletTailNodes = 64;

// One wave per record of order[begin, begin + count): its treelet restructured.
hipError_t launch_treelet_level(const TreeletArgs& a, const int32_t* order, int begin, int count, hipStream_t s);
// Levels [firstLevel, numLevels) in one workgroup, a barrier between levels; offsets: device
// int32[numLevels + 1] into order.
hipError_t launch_treelet_tail(const TreeletArgs& a, const int32_t* order, const int32_t* offsets, int firstLevel,
                               int numLevels, hipStream_t s);

}  // namespace mrt
