// wide_kernel.hpp — launch interface between the C-ABI glue (derive_api.cpp) and the gfx950
// kernels that derive the refit plan and the exact 4-wide array of a Compact2 tree on the
// device (wide_kernel.hip). The per-node steps are wide_common.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "wide_common.hpp"

namespace mrt {

// Depth levels of at most this many nodes are walked by one workgroup, consecutive ones in
// one launch with a barrier between them (launch_derive_chain), like the refit's tail.
constexpr int kDeriveChainNodes = 1024;

// The per-node steps a level launch can run (wide_common.hpp).
enum DeriveStep : int { kStepExpand, kStepHeight, kStepFlag, kStepSize, kStepIndex };

// Bytes of scratch the derivation of numNodes records needs (the sort's temporary storage
// included, asked of rocPRIM for the current device), and d's scratch pointers set into it:
// everything of wide::Derive but nodes, woopX, wideOut and srcOut. keysOut / ids are the
// sort's other buffers; depthOffsets holds maxLevels + 1 level starts.
struct DeriveScratch {
    int32_t* keysOut;
    int32_t* ids;
    int32_t* depthOffsets;
    void* primTemp;
    size_t primTempBytes;
};
hipError_t derive_scratch_bytes(int numNodes, int maxLevels, size_t* bytes, size_t* primTempBytes);
void derive_carve(wide::Derive& d, DeriveScratch& x, int numNodes, int maxLevels, void* scratch, size_t primTempBytes);

// Zeroes the flags and counters and seeds node 0 (wide_common.hpp, Derive).
hipError_t launch_derive_init(const wide::Derive& d, const DeriveScratch& x, hipStream_t s);
// Topology, one depth level: one thread per node of the frontier byDepth[begin, begin + count),
// which is depth level `level` (its start is written to depthOffsets[level]); the next
// frontier is byDepth[begin + count, summary[kReached]).
hipError_t launch_derive_expand(const wide::Derive& d, int32_t* depthOffsets, int level, int begin, int count,
                                hipStream_t s);
// Topology, in one workgroup: depth levels from `level` on while the frontier is neither empty
// nor above kDeriveChainNodes and the level is below maxLevels; summary[kNextLevel / kFrontBegin /
// kFrontEnd] say where it stopped. An empty frontier writes the last level's end.
hipError_t launch_derive_expand_chain(const wide::Derive& d, int32_t* depthOffsets, int level, int begin, int end,
                                      int maxLevels, hipStream_t s);
// One thread per node of byDepth[begin, begin + count): any step but kStepExpand.
hipError_t launch_derive_level(DeriveStep step, const wide::Derive& d, int begin, int count, hipStream_t s);
// Depth levels [first, last) in one workgroup, rising (dir > 0) or falling, a barrier between
// levels; depthOffsets: device int32 level starts into byDepth.
hipError_t launch_derive_chain(DeriveStep step, const wide::Derive& d, const int32_t* depthOffsets, int first,
                               int last, int dir, hipStream_t s);
// order = the node indices sorted by (height, index): a stable radix sort by height of the
// indices in ascending order (all 32 key bits, as the temporary storage was asked for);
// offsets[0 .. levels] = the level starts, read off the sorted heights (levels = node 0's
// height + 1; -1 stays where a height does not occur).
hipError_t launch_derive_sort(const wide::Derive& d, const DeriveScratch& x, int32_t* order, int32_t* offsets,
                              int levels, hipStream_t s);
// One thread per node: a wide root writes its 128-byte node and its four source slots.
hipError_t launch_derive_emit(const wide::Derive& d, hipStream_t s);

}  // namespace mrt
