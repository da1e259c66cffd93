// build_api.cpp — building an LBVH on the device into the caller's Compact2 buffers and binding
// it: mrt_tracer_build / _build_info and mrt_lbvh_sizes. The topology is lbvh_kernel.hip's, the
// Woop rows and boxes are the refit's launches (refit_api.cpp), the bind is bind_api.cpp's.
#include <string>

#include "lbvh_common.hpp"
#include "lbvh_kernel.hpp"
#include "refit_plan.hpp"
#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;

namespace {

int check_build_count(int64_t numTriangles) {
    if (numTriangles < 1) return fail(MRT_ERR_INVALID_ARG, "build: numTriangles < 1");
    if (numTriangles > mrt::lbvh::kMaxTriangles)
        return fail(MRT_ERR_TOO_LARGE, "build: more than 67108863 triangles (2^28 Woop slots, the refit's limit)");
    return MRT_OK;
}

// The stream-ordered scratch and the phase events of one build, returned on every way out.
struct BuildTemps {
    mrt::Event ev[5];
    mrt::StreamScratch scratch;   // last: freed on its stream before the events go
};

// mrt_tracer_build (onDevice false) and mrt_tracer_build_device: one sequence, the level plan and
// the bind's derived data made on the host or on the device (derive_api.cpp).
int build_impl(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
               int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity, void* woop,
               int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity, int64_t* nodeBytes,
               int64_t* woopBytes, int64_t* triIndexBytes, void* stream, bool onDevice);

}  // namespace

extern "C" {

int mrt_lbvh_sizes(int64_t numTriangles, int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes) {
    if (!nodeBytes || !woopBytes || !triIndexBytes) return fail(MRT_ERR_INVALID_ARG, "lbvh_sizes: null argument");
    if (int rc = check_build_count(numTriangles)) return rc;
    *nodeBytes = mrt::lbvh::max_records(numTriangles) * 64;
    *woopBytes = mrt::lbvh::max_slots(numTriangles) * 16;
    *triIndexBytes = mrt::lbvh::max_slots(numTriangles) * 4;
    return MRT_OK;
}

int mrt_tracer_build(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                     int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity,
                     void* woop, int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity,
                     int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes, void* stream) {
    return build_impl(t, vertices, numVertices, triangles, numTriangles, params, nodes, nodeCapacity, woop, woopCapacity,
                      triIndex, triIndexCapacity, nodeBytes, woopBytes, triIndexBytes, stream, false);
}

int mrt_tracer_build_device(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                            int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity,
                            void* woop, int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity,
                            int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes, void* stream) {
    return build_impl(t, vertices, numVertices, triangles, numTriangles, params, nodes, nodeCapacity, woop, woopCapacity,
                      triIndex, triIndexCapacity, nodeBytes, woopBytes, triIndexBytes, stream, true);
}

int mrt_tracer_build_info(mrt_tracer* t, mrt_build_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    *info = t->lastBuild;
    return MRT_OK;
}

}  // extern "C"

namespace {

int build_impl(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
               int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity, void* woop,
               int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity, int64_t* nodeBytes,
               int64_t* woopBytes, int64_t* triIndexBytes, void* stream, bool onDevice) {
    int maxLeaf = params ? params->max_leaf_size : 0;
    if (maxLeaf < 0 || maxLeaf > mrt::lbvh::kMaxLeafLimit) return fail(MRT_ERR_INVALID_ARG, "build: max_leaf_size outside 0..8");
    if (maxLeaf == 0) maxLeaf = MRT_LBVH_DEFAULT_MAX_LEAF;
    if (numVertices < 0) return fail(MRT_ERR_INVALID_ARG, "build: numVertices < 0");
    if (int rc = check_build_count(numTriangles)) return rc;
    if (!t || (numVertices && !vertices) || !triangles || !nodes || !woop || !triIndex || !nodeBytes || !woopBytes ||
        !triIndexBytes)
        return fail(MRT_ERR_INVALID_ARG, "build: null argument");
    const int n = (int)numTriangles;
    const int64_t maxRecords = mrt::lbvh::max_records(n), maxSlots = mrt::lbvh::max_slots(n);
    if (nodeCapacity < maxRecords * 64 || woopCapacity < maxSlots * 16 || triIndexCapacity < maxSlots * 4)
        return fail(MRT_ERR_TOO_LARGE, "build: an output capacity is below mrt_lbvh_sizes");

    std::lock_guard<std::mutex> lock(t->mu);
    DeviceGuard guard(t->device);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = static_cast<hipStream_t>(stream);

    // Scratch: the topology's (lbvh_kernel.hip), then the refit's valid flags, skipped
    // counter and level plan, each on a 256-byte boundary.
    size_t topoBytes = 0, primBytes = 0;
    MRT_HIP(mrt::lbvh_scratch_bytes(n, &topoBytes, &primBytes));
    auto aligned = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t validAt = aligned(topoBytes), skippedAt = validAt + aligned((size_t)maxRecords * 2),
                 orderAt = skippedAt + 256, offsetsAt = orderAt + aligned((size_t)maxRecords * 4),
                 total = offsetsAt + aligned(((size_t)maxRecords + 1) * 4);
    BuildTemps tmp;
    MRT_HIP(tmp.scratch.alloc(total, s));
    for (mrt::Event& e : tmp.ev) MRT_HIP(e.create());
    char* base = tmp.scratch.as<char>();
    auto* skippedDev = reinterpret_cast<unsigned long long*>(base + skippedAt);
    auto* orderDev = reinterpret_cast<int32_t*>(base + orderAt);
    auto* offsetsDev = reinterpret_cast<int32_t*>(base + offsetsAt);

    mrt::LbvhBuild b{};
    b.vertices = vertices;
    b.numVertices = numVertices;
    b.triangles = triangles;
    b.numTriangles = n;
    b.maxLeaf = maxLeaf;
    b.nodes = static_cast<uint32_t*>(nodes);
    b.woop = static_cast<uint32_t*>(woop);
    b.triIndex = triIndex;
    mrt::lbvh_carve(b, base, primBytes);

    // Phase 1: keys and order. Phase 2: hierarchy and emission.
    const bool single = n <= maxLeaf;
    MRT_HIP(hipEventRecord(tmp.ev[0], s));
    MRT_HIP(mrt::launch_lbvh_sort(b, s));
    MRT_HIP(hipEventRecord(tmp.ev[1], s));
    MRT_HIP(single ? mrt::launch_lbvh_emit_single(b, s) : mrt::launch_lbvh_emit(b, s));
    MRT_HIP(hipEventRecord(tmp.ev[2], s));
    int32_t records = 1, leaves = 2;
    if (!single) {
        MRT_HIP(hipMemcpyAsync(&records, b.keptRank + (n - 1), 4, hipMemcpyDeviceToHost, s));
        MRT_HIP(hipMemcpyAsync(&leaves, b.leafRank + n, 4, hipMemcpyDeviceToHost, s));
    }
    MRT_HIP(hipStreamSynchronize(s));
    if (records < 1 || records > maxRecords || leaves < 1 || leaves > n + 1)
        return fail(MRT_ERR_HIP, "build: the emitted counts are inconsistent");
    const int64_t slots = 3 * (int64_t)n + leaves;

    // The level plan of the emitted topology: on the device, kept as the tracer's refit plan, or
    // on the host (the call is synchronous for it; so above MRT_DERIVE_MAX_LEVELS depth levels).
    static const char* const kPrefix = "build: the emitted nodes are not a tree: ";
    const auto tPlan = std::chrono::steady_clock::now();
    mrt::Derivation d;
    mrt::RefitPlan& plan = d.plan;
    bool derived = false;
    if (onDevice) {
        if (int rc = mrt::derive(d, nodes, records, s, MRT_ERR_HIP, kPrefix)) return rc;
        derived = !d.tooDeep;
    }
    if (derived) {
        orderDev = plan.order.get();
        offsetsDev = plan.offsets.get();
        skippedDev = plan.skipped.get();
    } else {
        mrt::RefitLevels lv;
        if (int rc = mrt::host_levels(nodes, records, s, MRT_ERR_HIP, kPrefix, &lv)) return rc;
        if (int rc = mrt::upload_levels(lv, orderDev, offsetsDev, skippedDev, s)) return rc;
        plan.levels = lv.offsets;
    }
    const double planMs = mrt::ms_since(tPlan);

    // Phase 3: Woop rows and boxes, by the refit's launches on the buffers not yet bound.
    mrt::RefitArgs a{};
    a.nodes = b.nodes;
    a.numNodes = records;
    a.woop = b.woop;
    a.woopSlots = (int)slots;
    a.triIndex = triIndex;
    a.vertices = vertices;
    a.numVertices = numVertices;
    a.triangles = triangles;
    a.numTriangles = n;
    a.valid = derived ? plan.valid.get() : reinterpret_cast<uint8_t*>(base + validAt);
    a.skipped = skippedDev;
    int launches = 0;
    MRT_HIP(hipEventRecord(tmp.ev[3], s));
    if (int rc = mrt::enqueue_refit(a, plan.levels, orderDev, offsetsDev, s, &launches)) return rc;
    if (single) MRT_HIP(mrt::launch_lbvh_empty_leaf_box(b.nodes, s));
    MRT_HIP(hipEventRecord(tmp.ev[4], s));
    unsigned long long skipped = 0;
    MRT_HIP(hipMemcpyAsync(&skipped, skippedDev, sizeof(skipped), hipMemcpyDeviceToHost, s));
    if (derived) MRT_HIP(hipMemsetAsync(skippedDev, 0, sizeof(skipped), s));   // the kept plan counts refits only
    MRT_HIP(hipStreamSynchronize(s));

    mrt_build_info info{};
    MRT_HIP(hipEventElapsedTime(&info.sort_ms, tmp.ev[0], tmp.ev[1]));
    MRT_HIP(hipEventElapsedTime(&info.emit_ms, tmp.ev[1], tmp.ev[2]));
    MRT_HIP(hipEventElapsedTime(&info.fit_ms, tmp.ev[3], tmp.ev[4]));

    // The buffers are written: a bind that fails leaves the tracer unbound.
    const mrt::BvhBuffers built{nodes, (int64_t)records * 64, woop, slots * 16, triIndex, slots * 4};
    const int32_t levels = (int32_t)plan.levels.size() - 1;   // the install takes the plan
    if (int rc = mrt::install(t, built, onDevice ? &d : nullptr, s, mrt::kUnbindOnError)) return rc;
    info.plan_ms = planMs;
    info.bind_ms = t->bindMs;
    info.levels = levels;
    info.records = records;
    info.leaves = leaves;
    info.slots = slots;
    info.scratch_bytes = (int64_t)(total + d.run.scratchBytes);
    info.skipped_refs = (int64_t)skipped;
    info.max_leaf_size = maxLeaf;
    info.wall_ms = mrt::ms_since(t0);
    t->lastBuild = info;
    *nodeBytes = built.nodeBytes;
    *woopBytes = built.woopBytes;
    *triIndexBytes = built.triIndexBytes;
    return MRT_OK;
}

}  // namespace
