// raysort.cpp — the CPU statement of mrt_ray_sort (include/mrt.h, csrc/raysort_kernel.hip): the
// Morton sort of a ray batch, RayBuffer::mortonSort (reference RayBuffer.cc:256-324). The box, the
// keys and the order are raysort_common.hpp's, so keys, permutation, rays and id maps equal the
// device's bit for bit; the sort is std::stable_sort on the shifted key.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../../include/mrt_host.h"
#include "../raysort_common.hpp"
#include "host_error.hpp"

namespace rs = mrt::raysort;

extern "C" int mrth_ray_sort(const void* inRays, const int32_t* inSlotToId, int32_t numRays,
                             const mrth_ray_sort_params* params, void* outRays, int32_t* outIdToSlot,
                             int32_t* outSlotToId, uint32_t* outKeys, float* outBox) {
    const int dropLevels = params ? params->drop_levels : 0;
    const int box = params ? params->box : 0;
    if (numRays < 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "negative ray count");
    if (dropLevels < 0 || dropLevels > rs::kMaxDropLevels)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "drop_levels outside 0..24");
    if (box != 0 && box != 1) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "box outside 0..1");
    if (numRays == 0) return MRTH_OK;
    if (!inRays || !outRays) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "null rays");
    if (numRays > rs::kMaxRays) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "more than 2^30 rays");
    const uintptr_t in = reinterpret_cast<uintptr_t>(inRays), out = reinterpret_cast<uintptr_t>(outRays);
    const uintptr_t rayBytes = (uintptr_t)numRays * 32;
    if (in < out + rayBytes && out < in + rayBytes)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "outRays overlaps inRays");

    const size_t n = (size_t)numRays;
    const char* src = static_cast<const char*>(inRays);
    auto ray_at = [&](size_t i, float ray[8]) { std::memcpy(ray, src + i * 32, 32); };

    rs::Box all = rs::box_empty();
    for (size_t i = 0; i < n; i++) {
        float ray[8];
        ray_at(i, ray);
        rs::box_grow_ray(all, ray, box);
    }
    if (outBox)
        for (int k = 0; k < 3; k++) {
            outBox[k] = all.lo[k];
            outBox[3 + k] = all.hi[k];
        }

    std::vector<uint32_t> own;
    uint32_t* keys = outKeys;
    if (!keys) {
        own.resize(n * rs::kKeyWords);
        keys = own.data();
    }
    for (size_t i = 0; i < n; i++) {
        float ray[8];
        ray_at(i, ray);
        rs::ray_key(ray, all, keys + i * rs::kKeyWords);
    }

    const int passes = rs::sort_passes(dropLevels);
    std::vector<int32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) {
        for (int pass = passes - 1; pass >= 0; pass--) {
            const uint64_t wa = rs::shifted_word(keys + (size_t)a * rs::kKeyWords, dropLevels, pass);
            const uint64_t wb = rs::shifted_word(keys + (size_t)b * rs::kKeyWords, dropLevels, pass);
            if (wa != wb) return wa < wb;
        }
        return false;
    });

    char* dst = static_cast<char*>(outRays);
    for (size_t j = 0; j < n; j++) {
        const int32_t p = perm[j];
        std::memcpy(dst + j * 32, src + (size_t)p * 32, 32);
        const int32_t id = inSlotToId ? inSlotToId[p] : p;
        if (outSlotToId) outSlotToId[j] = id;
        if (outIdToSlot && (uint32_t)id < (uint32_t)numRays) outIdToSlot[id] = (int32_t)j;
    }
    return MRTH_OK;
}
