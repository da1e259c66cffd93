// raysort_api.cpp — the C-ABI of the device ray sort: mrt_ray_sort. The argument checks, the
// stream-ordered scratch, the launches (raysort_kernel.hip). Everything is enqueued on the caller's
// stream; nothing waits on the host, nothing is read back and no state outlives the call.
//
//   mrt_ray_sort  <- RayBuffer::mortonSort (reference RayBuffer.cc:256-324), which copies the keys
//                    to the host, sorts them there and copies them back
#include <string>

#include "api_common.hpp"
#include "raysort_kernel.hpp"

using mrt::fail;
using mrt::hipFail;

extern "C" {

int mrt_ray_sort(const void* inRays, const int32_t* inSlotToId, int32_t numRays, const mrt_ray_sort_params* params,
                 void* outRays, int32_t* outIdToSlot, int32_t* outSlotToId, uint32_t* outKeys, float* outBox,
                 void* stream) {
    const int dropLevels = params ? params->drop_levels : 0;
    const int boxMode = params ? params->box : 0;
    if (numRays < 0) return fail(MRT_ERR_INVALID_ARG, "negative ray count");
    if (dropLevels < 0 || dropLevels > mrt::raysort::kMaxDropLevels)
        return fail(MRT_ERR_INVALID_ARG, "drop_levels outside 0..24");
    if (boxMode != 0 && boxMode != 1) return fail(MRT_ERR_INVALID_ARG, "box outside 0..1");
    if (numRays == 0) return MRT_OK;
    if (!inRays || !outRays) return fail(MRT_ERR_INVALID_ARG, "null rays");
    if (numRays > mrt::raysort::kMaxRays) return fail(MRT_ERR_TOO_LARGE, "more than 2^30 rays");
    const uintptr_t in = reinterpret_cast<uintptr_t>(inRays), out = reinterpret_cast<uintptr_t>(outRays);
    const uintptr_t rayBytes = (uintptr_t)numRays * 32;
    if (in < out + rayBytes && out < in + rayBytes) return fail(MRT_ERR_INVALID_ARG, "outRays overlaps inRays");

    hipStream_t s = static_cast<hipStream_t>(stream);
    mrt::RaySort a{};
    a.inRays = static_cast<const uint4*>(inRays);
    a.inSlotToId = inSlotToId;
    a.numRays = numRays;
    a.dropLevels = dropLevels;
    a.boxMode = boxMode;
    a.outRays = static_cast<uint4*>(outRays);
    a.outIdToSlot = outIdToSlot;
    a.outSlotToId = outSlotToId;
    a.keys = outKeys;
    a.box = outBox;
    size_t bytes = 0, primTempBytes = 0;
    if (hipError_t e = mrt::raysort_scratch_bytes(numRays, dropLevels, !outKeys, !outBox, &bytes, &primTempBytes))
        return hipFail(e, "rocprim::radix_sort_pairs(size query)");
    mrt::StreamScratch scratch;
    if (hipError_t e = scratch.alloc(bytes, s)) return hipFail(e, "hipMallocAsync(ray sort scratch)");
    mrt::raysort_carve(a, scratch.p, primTempBytes);
    const hipError_t launch = mrt::launch_raysort(a, s);
    const hipError_t f = scratch.release();
    if (launch != hipSuccess) return hipFail(launch, "ray sort launch");
    return f == hipSuccess ? MRT_OK : hipFail(f, "hipFreeAsync(ray sort scratch)");
}

}  // extern "C"
