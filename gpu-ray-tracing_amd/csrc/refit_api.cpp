// refit_api.cpp — refitting a bound BVH on the device for moved vertices (fixed topology):
// the plan (the nodes by height level, refit_plan.cpp) and the launches (refit_kernel.hip) behind
// mrt_tracer_refit / _refit_info, and the host-only mrt_refit_plan.
#include <cstring>
#include <string>

#include "refit_plan.hpp"
#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;

namespace mrt {

// Device-wide, like workspace_wait: the refit's stream is the caller's and may be gone.
int wait_refit(mrt_tracer* t) {
    if (t->plan.launched) MRT_HIP(hipDeviceSynchronize());
    t->plan.launched = false;
    return MRT_OK;
}

int host_levels(const void* nodes, int64_t numNodes, hipStream_t s, int code, const char* prefix, RefitLevels* lv) {
    std::vector<int32_t> host((size_t)numNodes * 16);
    MRT_HIP(hipMemcpyAsync(host.data(), nodes, host.size() * 4, hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));
    if (const char* why = refit_levels(host.data(), numNodes, lv)) return fail(code, std::string(prefix) + why);
    return MRT_OK;
}

int upload_levels(const RefitLevels& lv, int32_t* order, int32_t* offsets, unsigned long long* skipped, hipStream_t s) {
    const std::vector<int32_t> offsets32(lv.offsets.begin(), lv.offsets.end());   // < 2^26 nodes
    MRT_HIP(hipMemcpyAsync(order, lv.order.data(), lv.order.size() * 4, hipMemcpyHostToDevice, s));
    MRT_HIP(hipMemcpyAsync(offsets, offsets32.data(), offsets32.size() * 4, hipMemcpyHostToDevice, s));
    MRT_HIP(hipMemsetAsync(skipped, 0, sizeof(unsigned long long), s));
    MRT_HIP(hipStreamSynchronize(s));   // the uploads read lv and offsets32
    return MRT_OK;
}

namespace {

// Builds the refit plan of the bound tree (the handle's mutex held) on the device
// (derive_api.cpp: no node array crosses to the host). Synchronous. A tree of more than
// MRT_DERIVE_MAX_LEVELS depth levels takes the host path: the Compact2 nodes come to the host
// once for their child refs (topology only: a refit in flight changes boxes, never words 12-15).
int build_plan(mrt_tracer* t) {
    if (t->plan.built) return MRT_OK;
    static const char* const kPrefix = "refit: the bound nodes are not a tree: ";
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t numNodes = t->bvh.numNodes();
    Derivation d;
    RefitPlan& p = d.plan;
    mrt_derive_info info{};
    if (int rc = derive(d, t->bvh.nodes, numNodes, nullptr, MRT_ERR_INVALID_ARG, kPrefix)) return rc;
    if (d.tooDeep) {
        RefitLevels lv;
        if (int rc = host_levels(t->bvh.nodes, numNodes, nullptr, MRT_ERR_INVALID_ARG, kPrefix, &lv)) return rc;
        MRT_HIP(p.order.alloc(lv.order.size() * 4));
        MRT_HIP(p.offsets.alloc(lv.offsets.size() * 4));
        MRT_HIP(p.valid.alloc((size_t)numNodes * 2));
        MRT_HIP(p.skipped.alloc(sizeof(unsigned long long)));
        if (int rc = upload_levels(lv, p.order.get(), p.offsets.get(), p.skipped.get(), nullptr)) return rc;
        p.bytes = (int64_t)lv.order.size() * 4 + (int64_t)lv.offsets.size() * 4 + numNodes * 2 + 8;
        p.levels = lv.offsets;
    }
    MRT_HIP(hipStreamSynchronize(nullptr));   // the offsets' upload reads d.run
    if (int rc = derive_report(d.run, !d.tooDeep, false, &info)) return rc;   // too deep: the info says so
    p.built = true;
    Install in;
    in.plan = &p;   // complete, or not held at all
    in.derive = &info;
    in.since = &t0;
    in.keepTunes = true;
    return commit(t, t->bvh, in);
}

}  // namespace

// The Woop rows and boxes of the Compact2 buffers in `a`, bound or not: the leaves, then the
// inner levels (walk_levels above kRefitTailNodes nodes). levelOffsets: the plan's offsets on
// the host; order / offsets: the plan on the device.
int enqueue_refit(const RefitArgs& a, const std::vector<int64_t>& levelOffsets, const int32_t* order,
                  const int32_t* offsets, hipStream_t s, int* launches) {
    MRT_HIP(launch_refit_leaves(a, s));
    ++*launches;
    return walk_levels(
        levelOffsets, kRefitTailNodes, launches,
        [&](int begin, int count) { return launch_refit_level(a, order, begin, count, s); },
        [&](int first, int levels) { return launch_refit_tail(a, order, offsets, first, levels, s); });
}

}  // namespace mrt

extern "C" {

int mrt_tracer_refit(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                     int64_t numTriangles, void* stream) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    if (numVertices < 0 || numTriangles < 0 || (numVertices && !vertices) || (numTriangles && !triangles))
        return fail(MRT_ERR_INVALID_ARG, "refit: bad vertex / triangle arrays");
    std::lock_guard<std::mutex> lock(t->mu);
    if (!t->bvh) return fail(MRT_ERR_NOT_BOUND, "refit before bind (no BVH)");
    DeviceGuard guard(t->device);
    if (int rc = mrt::build_plan(t)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mrt::RefitPlan& plan = t->plan;
    mrt::WideArray& wide = t->wide;

    mrt::RefitArgs a{};
    a.nodes = static_cast<uint32_t*>(const_cast<void*>(t->bvh.nodes));   // refit writes the bound buffers (mrt.h)
    a.numNodes = (int)t->bvh.numNodes();
    a.woop = static_cast<uint32_t*>(const_cast<void*>(t->bvh.woop));
    a.woopSlots = (int)(t->bvh.woopBytes / 16);
    a.triIndex = t->bvh.triIndex;
    a.vertices = vertices;
    a.numVertices = numVertices;
    a.triangles = triangles;
    a.numTriangles = numTriangles;
    a.valid = plan.valid.get();
    a.skipped = plan.skipped.get();

    int launches = 0;
    plan.launched = true;
    if (int rc = mrt::enqueue_refit(a, plan.levels, plan.order.get(), plan.offsets.get(), s, &launches)) return rc;
    if (wide.src) {
        MRT_HIP(mrt::launch_refit_wide(a, wide.src.get(), wide.nodes.get(), (int)(wide.bytes / 128), s));
        launches++;
    }
    plan.launches = launches;
    if (wide.nodes && wide.format == mrt::kNodeWide4Q) {
        // The quantized form has no in-place update: derive it again from the refitted
        // nodes through the bind-time host path (synchronous and slow; mrt.h).
        // (Should a box no longer quantize, the exact form comes back and the commit puts its
        // source map on the device beside the plan.)
        MRT_HIP(hipStreamSynchronize(s));
        return mrt::refresh_wide(t, true);
    }
    return MRT_OK;
}

int mrt_tracer_refit_info(mrt_tracer* t, mrt_refit_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    std::memset(info, 0, sizeof(*info));
    if (!t->plan.built) return MRT_OK;
    DeviceGuard guard(t->device);
    if (int rc = mrt::wait_refit(t)) return rc;
    unsigned long long skipped = 0;
    MRT_HIP(hipMemcpy(&skipped, t->plan.skipped.get(), sizeof(skipped), hipMemcpyDeviceToHost));
    MRT_HIP(hipMemset(t->plan.skipped.get(), 0, sizeof(skipped)));
    info->levels = (int32_t)t->plan.levels.size() - 1;
    info->launches = t->plan.launches;
    info->plan_bytes = t->plan.bytes + t->wide.srcBytes();
    info->skipped_refs = (int64_t)skipped;
    return MRT_OK;
}

int mrt_refit_plan(const void* nodes, int64_t nodeBytes, int32_t* order, int64_t* levelOffsets, int32_t levelCapacity,
                   int32_t* numLevels, int32_t* wideSrc, int64_t wideSrcCapacity, int64_t* numWideSrc) {
    if (!nodes || nodeBytes <= 0 || nodeBytes % 64 != 0 || !numLevels || levelCapacity < 0 || wideSrcCapacity < 0)
        return fail(MRT_ERR_INVALID_ARG, "refit_plan: bad arguments");
    const auto* n = static_cast<const int32_t*>(nodes);
    mrt::RefitLevels lv;
    if (const char* why = mrt::refit_levels(n, nodeBytes / 64, &lv))
        return fail(MRT_ERR_INVALID_ARG, std::string("refit_plan: ") + why);
    *numLevels = lv.levels();
    if (order) std::memcpy(order, lv.order.data(), lv.order.size() * 4);
    if (levelOffsets) {
        if (levelCapacity < (int32_t)lv.offsets.size()) return fail(MRT_ERR_TOO_LARGE, "refit_plan: levelOffsets too small");
        std::memcpy(levelOffsets, lv.offsets.data(), lv.offsets.size() * 8);
    }
    if (numWideSrc) {
        std::vector<int32_t> src;
        (void)mrt::build_wide4(n, nodeBytes / 64, nullptr, 0, &src);
        *numWideSrc = (int64_t)src.size();
        if (wideSrc) {
            if (wideSrcCapacity < *numWideSrc) return fail(MRT_ERR_TOO_LARGE, "refit_plan: wideSrc too small");
            std::memcpy(wideSrc, src.data(), src.size() * 4);
        }
    }
    return MRT_OK;
}

}  // extern "C"
