// raysort_kernel.hpp — launch interface between the C-ABI glue (raysort_api.cpp, compat_api.cpp)
// and the gfx950 kernels that sort a ray batch by its Morton key (raysort_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "raysort_common.hpp"

namespace mrt {

constexpr int kRaySortBoxBlocks = 1024;   // at most this many partial boxes (6 floats each)

// One sort's inputs, outputs and scratch (all device pointers).
struct RaySort {
    const uint4* inRays;         // two per ray
    const int32_t* inSlotToId;   // NULL = identity
    int numRays;                 // 1 .. raysort::kMaxRays
    int dropLevels;              // 0 .. raysort::kMaxDropLevels
    int boxMode;                 // 0 = origins and end points, 1 = origins
    uint4* outRays;
    int32_t* outIdToSlot;        // may be NULL
    int32_t* outSlotToId;        // may be NULL
    uint32_t* keys;              // 6 per ray, input order: the caller's or scratch
    float* box;                  // lo.xyz, hi.xyz: the caller's or scratch
    // Scratch (raysort_carve).
    float* partial;              // 6 per block of the box launch
    uint64_t* word;              // a pass's 64-bit word per position, then sorted
    uint64_t* wordSorted;
    int32_t* perm;               // the permutation before and after a pass
    int32_t* permSorted;
    void* primTemp;              // the sort's temporary storage
    size_t primTempBytes;
};

// Bytes of scratch a sort of numRays needs (rocPRIM's temporary storage included, asked for the
// current device), with room for the keys and the box when the caller gives none; and s's scratch
// pointers (keys and box too, where they are NULL) set into it.
hipError_t raysort_scratch_bytes(int numRays, int dropLevels, bool ownKeys, bool ownBox, size_t* bytes,
                                 size_t* primTempBytes);
void raysort_carve(RaySort& s, void* scratch, size_t primTempBytes);

// The whole sort: box, keys, the passes, the reorder.
hipError_t launch_raysort(const RaySort& s, hipStream_t stream);

// The steps on their own (the reference's three launchers). partial: 6 * kRaySortBoxBlocks floats.
hipError_t launch_raysort_box(const uint4* rays, int numRays, int boxMode, float* partial, float* box, hipStream_t stream);
// out[stride * i + stride - 6 ..] = ray i's key; stride 7 also writes out[7 i] = i (MortonKey). The
// box is read from boxDev when that is not NULL, else taken from boxHost.
hipError_t launch_raysort_keys(const uint4* rays, int numRays, const float* boxDev, const raysort::Box& boxHost,
                               uint32_t* out, int stride, hipStream_t stream);
// outRays[j] = inRays[perm[permStride * j]] and the id maps.
hipError_t launch_raysort_reorder(const uint4* inRays, const int32_t* inSlotToId, int numRays, const int32_t* perm,
                                  int permStride, uint4* outRays, int32_t* outIdToSlot, int32_t* outSlotToId,
                                  hipStream_t stream);

}  // namespace mrt
