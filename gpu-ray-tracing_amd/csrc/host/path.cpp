// path.cpp — a path frame's vertex step, accumulation and resolve on the CPU: the statements
// mrt_path_extend / _accumulate / _resolve (csrc/path_kernel.hip) are checked against, term for
// term (csrc/path_common.hpp). The slots are walked in order, so a survivor's compacted place is
// the running count of survivors before it: the definition the device's count, scan and ballot give.
#include <cstring>

#include "../../../include/mrt_host.h"
#include "../path_common.hpp"
#include "../path_plan.hpp"
#include "host_error.hpp"
#include "records.hpp"

namespace mrt {
namespace {

static_assert(sizeof(rg::RayRec) == 32 && sizeof(path::State) == 16, "record sizes");

struct Pending {
    float v[4];
};

void add3(float* radiance, int32_t task, const float v[3]) {
    for (int c = 0; c < 3; c++) radiance[4 * (int64_t)task + c] += v[c];
}

}  // namespace

void path_extend(const mrth_path_extend_params& a) {
    path::Params p;
    p.vertex = a.vertex;
    p.depth = a.depth;
    p.numSamples = a.numSamples;
    p.seed = a.seed;
    for (int k = 0; k < 3; k++) {
        p.lightPos[k] = a.lightPos[k];
        p.lightColor[k] = a.lightColor[k];
        p.sky[k] = a.sky[k];
    }
    p.lightRadius = a.lightRadius;
    p.maxDist = a.maxDist;
    p.triNormals = a.triNormals;
    p.triMaterialColor = a.triMaterialColor;
    p.numTris = a.numTris;
    int32_t survivors = 0;
    for (int32_t slot = 0; slot < a.numSlots; slot++) {
        path::State state = path::first_state(slot);
        int64_t at = slot;
        bool live = true;
        if (a.vertex == 0) {
            at = slot / a.numSamples;
        } else {
            state = get_record<path::State>(a.inState, slot);
            live = path::owns(state.task, a.numPaths);
        }
        path::Step st;
        st.survivor = st.escaped = false;
        if (live) {
            const RayResult res = get_record<RayResult>(a.inResults, at);
            path::extend(p, get_record<rg::RayRec>(a.inRays, at), res.id, res.t, state, st);
        }
        if (live && st.survivor) {
            const int64_t dest = a.compact ? survivors : slot;
            put_record(a.outShadowRays, dest, st.shadow);
            put_record(a.outPending, dest, Pending{{st.pending[0], st.pending[1], st.pending[2], 0.0f}});
            if (a.vertex < a.depth) put_record(a.outRays, dest, st.bounce);
            put_record(a.outState, dest, st.state);
            survivors++;
        } else if (!a.compact) {
            put_record(a.outShadowRays, slot, path::dead_ray());
            put_record(a.outPending, slot, Pending{{0.0f, 0.0f, 0.0f, 0.0f}});
            if (a.vertex < a.depth) put_record(a.outRays, slot, path::dead_ray());
            put_record(a.outState, slot, path::dead_state());
        }
        if (live && st.escaped) add3(a.radiance, st.task, st.add);
    }
    *a.liveCount = survivors;
}

}  // namespace mrt

extern "C" {

int mrth_path_extend(const mrth_path_extend_params* a) {
    if (!a) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "path_extend: null params");
    const mrt::PathPlan plan = mrt::plan_path_extend(a->vertex, a->depth, a->numSamples, a->numSlots, a->numPaths);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    if (plan.empty) return MRTH_OK;
    if (!a->triNormals || !a->triMaterialColor || !a->inRays || !a->inResults || (a->vertex > 0 && !a->inState) ||
        !a->outShadowRays || !a->outPending || (a->vertex < a->depth && !a->outRays) || !a->outState || !a->radiance ||
        !a->liveCount)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "path_extend: null argument");
    if (a->numTris < 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "path_extend: negative triangle count");
    mrt::path_extend(*a);
    return MRTH_OK;
}

int mrth_path_accumulate(int32_t numSlots, int32_t numPaths, const void* state, const void* pending,
                         const void* shadowResults, float* radiance) {
    const mrt::PathPlan plan = mrt::plan_path_accumulate(numSlots, numPaths);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    if (plan.empty) return MRTH_OK;
    if (!state || !pending || !shadowResults || !radiance)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "path_accumulate: null argument");
    for (int32_t slot = 0; slot < numSlots; slot++) {
        const int32_t task = mrt::get_record<mrt::path::State>(state, slot).task;
        if (!mrt::path::owns(task, numPaths) || mrt::get_record<mrt::RayResult>(shadowResults, slot).id != -1) continue;
        const mrt::Pending p = mrt::get_record<mrt::Pending>(pending, slot);
        mrt::add3(radiance, task, p.v);
    }
    return MRTH_OK;
}

int mrth_path_resolve(int32_t numSamples, int32_t firstPrimary, int32_t numPrimary, const int32_t* primarySlotToId,
                      const void* primaryResults, const float* radiance, uint32_t* pixels, float* image) {
    const mrt::PathPlan plan = mrt::plan_path_resolve(numSamples, firstPrimary, numPrimary);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    if (plan.empty) return MRTH_OK;
    if (!primarySlotToId || !primaryResults || !radiance || !pixels)
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "path_resolve: null argument");
    for (int64_t i = 0; i < numPrimary; i++) {
        const int64_t slot = firstPrimary + i;
        const int32_t pixel = primarySlotToId[slot];
        float v[4];
        if (mrt::get_record<mrt::RayResult>(primaryResults, slot).id == -1) mrt::path::background(v);
        else mrt::path::resolve_one(radiance + 4 * i * numSamples, numSamples, v);
        pixels[pixel] = mrt::light::to_abgr(v);
        if (image)
            for (int c = 0; c < 4; c++) image[4 * (int64_t)pixel + c] = v[c];
    }
    return MRTH_OK;
}

}  // extern "C"
