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

// bind, unbind, set_config, destroy and build_plan.
void drop_plan(mrt_tracer* t) {
    (void)wait_refit(t);   // a refit may still read the plan
    t->plan = RefitPlan{};
}

namespace {

template <class T>
int upload(DeviceBuf<T>* dst, const std::vector<T>& src) {
    MRT_HIP(dst->alloc(src.size() * sizeof(T)));
    MRT_HIP(hipMemcpy(dst->get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return MRT_OK;
}

// The wide source map of a host-derived exact array goes to the device with the plan; a
// device-derived one is there already (WideArray::srcDev).
int attach_wide_src(const mrt_tracer* t, RefitPlan* p) {
    const WideArray& w = t->wide;
    if (w.nodes && w.format == kNodeWide4 && (int64_t)w.src.size() == w.bytes / 128 * 4) {
        if (int rc = upload(&p->wideSrc, w.src)) return rc;
        p->bytes += (int64_t)w.src.size() * 4;
    } else if (w.nodes && w.format == kNodeWide4 && w.srcDev) {
        p->bytes += w.bytes / 128 * 4 * 4;
    }
    return MRT_OK;
}

// Builds the refit plan of the bound tree (the handle's mutex held) on the device
// (derive_api.cpp: no node array crosses to the host). Synchronous. A tree of more than
// MRT_DERIVE_MAX_LEVELS depth levels takes the host path: the Compact2 nodes come to the host
// once for their child refs (topology only: a refit in flight changes boxes, never words 12-15).
int build_plan(mrt_tracer* t) {
    if (t->plan.built) return MRT_OK;
    const int64_t numNodes = t->nodeBytes / 64;
    {
        const auto t0 = std::chrono::steady_clock::now();
        DeriveRun r;
        RefitPlan p;
        int status = kDeriveOk;
        const char* why = nullptr;
        if (int rc = derive_begin(r, t->nodes, numNodes, nullptr)) return rc;
        if (int rc = derive_plan(r, &p, nullptr, &status, &why)) return rc;
        if (status == kDeriveMalformed)
            return fail(MRT_ERR_INVALID_ARG, std::string("refit: the bound nodes are not a tree: ") + why);
        if (status == kDeriveOk) {
            MRT_HIP(hipStreamSynchronize(nullptr));   // the offsets' upload reads r
            drop_plan(t);
            if (int rc = attach_wide_src(t, &p)) return rc;
            p.built = true;
            t->plan = std::move(p);   // complete, or not held at all
            return derive_report(t, r, true, false, ms_since(t0));
        }
    }
    std::vector<int32_t> host((size_t)(t->nodeBytes / 4));
    MRT_HIP(hipMemcpy(host.data(), t->nodes, (size_t)t->nodeBytes, hipMemcpyDeviceToHost));
    RefitLevels lv;
    if (const char* why = refit_levels(host.data(), numNodes, &lv))
        return fail(MRT_ERR_INVALID_ARG, std::string("refit: the bound nodes are not a tree: ") + why);
    const std::vector<int32_t> offsets(lv.offsets.begin(), lv.offsets.end());   // < 2^26 nodes
    drop_plan(t);
    RefitPlan p;
    if (int rc = upload(&p.order, lv.order)) return rc;
    if (int rc = upload(&p.offsets, offsets)) return rc;
    MRT_HIP(p.valid.alloc((size_t)numNodes * 2));
    MRT_HIP(p.skipped.alloc(sizeof(unsigned long long)));
    MRT_HIP(hipMemset(p.skipped.get(), 0, sizeof(unsigned long long)));
    p.bytes = (int64_t)lv.order.size() * 4 + (int64_t)offsets.size() * 4 + numNodes * 2 + 8;
    if (int rc = attach_wide_src(t, &p)) return rc;
    p.levels = lv.offsets;
    p.built = true;
    t->plan = std::move(p);   // complete, or not held at all
    return MRT_OK;
}

}  // namespace

// The Woop rows and boxes of the Compact2 buffers in `a`, bound or not: the leaves, one launch
// per level above kRefitTailNodes nodes, one workgroup for all smaller levels. levels: the
// plan's offsets on the host; order / offsets: the plan on the device.
int enqueue_refit(const RefitArgs& a, const std::vector<int64_t>& levelOffsets, const int32_t* order,
                  const int32_t* offsets, hipStream_t s, int* launches) {
    MRT_HIP(launch_refit_leaves(a, s));
    ++*launches;
    const int levels = (int)levelOffsets.size() - 1;
    for (int l = 1; l < levels; l++) {
        const int begin = (int)levelOffsets[(size_t)l], count = (int)(levelOffsets[(size_t)l + 1] - begin);
        if (count > kRefitTailNodes) {
            MRT_HIP(launch_refit_level(a, order, begin, count, s));
            ++*launches;
            continue;
        }
        // level sizes never grow with the height: this one and all above it fit one workgroup
        MRT_HIP(launch_refit_tail(a, order, offsets, l, levels, s));
        ++*launches;
        break;
    }
    return MRT_OK;
}

}  // namespace mrt

extern "C" {

int mrt_tracer_refit(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                     int64_t numTriangles, void* stream) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    if (numVertices < 0 || numTriangles < 0 || (numVertices && !vertices) || (numTriangles && !triangles))
        return fail(MRT_ERR_INVALID_ARG, "refit: bad vertex / triangle arrays");
    std::lock_guard<std::mutex> lock(t->mu);
    if (!t->bound) return fail(MRT_ERR_NOT_BOUND, "refit before bind (no BVH)");
    DeviceGuard guard(t->device);
    if (int rc = mrt::build_plan(t)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mrt::RefitPlan& plan = t->plan;
    mrt::WideArray& wide = t->wide;

    mrt::RefitArgs a{};
    a.nodes = static_cast<uint32_t*>(const_cast<void*>(t->nodes));   // refit writes the bound buffers (mrt.h)
    a.numNodes = (int)(t->nodeBytes / 64);
    a.woop = static_cast<uint32_t*>(const_cast<void*>(t->woop));
    a.woopSlots = (int)(t->woopBytes / 16);
    a.triIndex = t->triIndex;
    a.vertices = vertices;
    a.numVertices = numVertices;
    a.triangles = triangles;
    a.numTriangles = numTriangles;
    a.valid = plan.valid.get();
    a.skipped = plan.skipped.get();

    int launches = 0;
    plan.launched = true;
    if (int rc = mrt::enqueue_refit(a, plan.levels, plan.order.get(), plan.offsets.get(), s, &launches)) return rc;
    if (const int32_t* wideSrc = mrt::refit_wide_src(t)) {
        MRT_HIP(mrt::launch_refit_wide(a, wideSrc, wide.nodes.get(), (int)(wide.bytes / 128), s));
        launches++;
    }
    plan.launches = launches;
    if (wide.nodes && wide.format == mrt::kNodeWide4Q) {
        // The quantized form has no in-place update: derive it again from the refitted
        // nodes through the bind-time host path (synchronous and slow; mrt.h).
        MRT_HIP(hipStreamSynchronize(s));
        wide.builtFor = -1;
        if (int rc = mrt::refresh_wide(t)) return rc;
        // the exact form as a fallback would need a new source map on the device
        if (wide.format == mrt::kNodeWide4) {
            plan.built = false;
            return mrt::build_plan(t);
        }
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
    info->plan_bytes = t->plan.bytes;
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
