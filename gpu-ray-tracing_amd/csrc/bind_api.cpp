// bind_api.cpp — binding a Compact2 BVH to a tracer and deriving its 4-wide nodes
// (wide_bvh.cpp): mrt_tracer_bind / _unbind / _bind_info / _copy_wide_nodes and the host-only
// mrt_derive_wide_nodes. The library borrows the bound buffers; the wide array is its own.
#include <algorithm>
#include <cstring>

#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;

namespace mrt {

// Synchronous (bind-time work: the Compact2 nodes come to the host, collapse, go back).
int refresh_wide(mrt_tracer* t) {
    const int want = t->bound ? t->cfg.wide : 0;
    if (want == t->wide.builtFor) return MRT_OK;
    DeviceGuard guard(t->device);
    // launches in flight may still read the old array: wait for this handle's own
    if (int rc = wait_all_workspaces(t)) return rc;
    if (int rc = wait_refit(t)) return rc;   // a refit's gather may still write it
    MRT_HIP(t->wide.nodes.free());
    t->wide = WideArray{};
    if (want) {
        std::vector<int32_t> host((size_t)(t->nodeBytes / 4));
        MRT_HIP(hipMemcpy(host.data(), t->nodes, (size_t)t->nodeBytes, hipMemcpyDeviceToHost));
        // The first word of every Woop slot (the terminators): the leaf refs carry counts.
        const int64_t slots = t->woopBytes / 16;
        const bool counts = leaf_counts_fit(slots);
        std::vector<int32_t> woopX;
        if (counts) {
            woopX.resize((size_t)slots);
            MRT_HIP(hipMemcpy2D(woopX.data(), 4, t->woop, 16, 4, (size_t)slots, hipMemcpyDeviceToHost));
        }
        const int32_t* wx = counts ? woopX.data() : nullptr;
        WideArray w;
        std::vector<uint32_t> wide;
        w.format = kNodeWide4;
        // The quantized form when asked for and every box quantizes; else the exact one.
        if (want == 2 && build_wide4q(host.data(), t->nodeBytes / 64, &wide, wx, slots)) w.format = kNodeWide4Q;
        else wide = build_wide4(host.data(), t->nodeBytes / 64, wx, slots, &w.src);
        w.leafCounts = counts;
        const int nodeWords = w.format == kNodeWide4 ? 32 : 16;
        const int64_t need = wide_stack_bound(wide.data(), (int64_t)wide.size() / nodeWords, nodeWords);
        if (need + 1 > kMaxWideStack) {   // a degenerate tree: keep the binary traversal and its reference capacity
            t->wide.builtFor = want;
            return MRT_OK;
        }
        w.stackCap = std::max<int>(kStackCapacity, (int)need + 1);
        w.stackBound = (int)need;
        w.bytes = (int64_t)wide.size() * 4;
        if (w.bytes > kMaxBufferBytes) return fail(MRT_ERR_TOO_LARGE, "4-wide node array above the 32-bit range");
        MRT_HIP(w.nodes.alloc((size_t)w.bytes));
        MRT_HIP(hipMemcpy(w.nodes.get(), wide.data(), (size_t)w.bytes, hipMemcpyHostToDevice));
        t->wide = std::move(w);   // complete, or not held at all
    }
    t->wide.builtFor = want;
    return MRT_OK;
}

int bind_locked(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                const int32_t* triIndex, int64_t triIndexBytes) {
    t->nodes = nodes;
    t->nodeBytes = nodeBytes;
    t->woop = woop;
    t->woopBytes = woopBytes;
    t->triIndex = triIndex;
    t->triIndexBytes = triIndexBytes;
    t->bound = true;
    t->wide.builtFor = -1;   // a new BVH: its wide nodes are derived now (if configured)
    DeviceGuard guard(t->device);
    tune_reset(t);           // and its schedules are tuned again
    drop_plan(t);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = refresh_wide(t);
    t->bindMs = ms_since(t0);
    return rc;
}

// mrt_tracer_bind's and mrt_tracer_bind_device's argument checks.
int check_bind_args(const mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                    const int32_t* triIndex, int64_t triIndexBytes) {
    if (!t || !nodes || !woop || !triIndex) return fail(MRT_ERR_INVALID_ARG, "null BVH buffer");
    if (nodeBytes < 64 || woopBytes < 16 || triIndexBytes < 4 || (nodeBytes % 64) || (woopBytes % 16) ||
        (triIndexBytes % 4))
        return fail(MRT_ERR_INVALID_ARG, "BVH buffer sizes are not Compact2-shaped");
    if (nodeBytes > kMaxBufferBytes || woopBytes > kMaxBufferBytes)
        return fail(MRT_ERR_TOO_LARGE, "Compact2 buffer above the 32-bit buffer-offset range");
    if (triIndexBytes / 4 != woopBytes / 16) return fail(MRT_ERR_INVALID_ARG, "triIndex must hold one int per woop float4");
    return MRT_OK;
}

// A device bind that refuses its tree leaves the tracer like this too; errors are dropped there.
void unbind_locked(mrt_tracer* t) {
    t->bound = false;
    t->nodes = t->woop = nullptr;
    t->triIndex = nullptr;
    DeviceGuard guard(t->device);
    drop_plan(t);
    t->wide.builtFor = -1;
    (void)refresh_wide(t);
}

}  // namespace mrt

extern "C" {

int mrt_tracer_bind(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                    const int32_t* triIndex, int64_t triIndexBytes) {
    if (int rc = mrt::check_bind_args(t, nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes)) return rc;
    std::lock_guard<std::mutex> lock(t->mu);
    return mrt::bind_locked(t, nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes);
}

int mrt_tracer_unbind(mrt_tracer* t) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    std::lock_guard<std::mutex> lock(t->mu);
    t->bound = false;
    t->nodes = t->woop = nullptr;
    t->triIndex = nullptr;
    DeviceGuard guard(t->device);
    mrt::drop_plan(t);
    return mrt::refresh_wide(t);
}

int mrt_tracer_bind_info(const mrt_tracer* t, mrt_bind_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    const mrt::WideArray& w = t->wide;
    info->bind_ms = t->bindMs;
    info->wide_bytes = w.nodes ? w.bytes : 0;
    info->wide_format = w.nodes ? w.format : mrt::kNodeCompact2;
    info->stack_capacity = w.nodes ? w.stackCap : mrt::kStackCapacity;
    info->stack_bound = w.nodes ? w.stackBound : mrt::kStackCapacity - 1;
    return MRT_OK;
}

int mrt_tracer_copy_wide_nodes(mrt_tracer* t, void* out, int64_t capacity, int64_t* bytes) {
    if (!t || !bytes) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    *bytes = t->wide.nodes ? t->wide.bytes : 0;
    if (!out || *bytes == 0) return MRT_OK;
    if (capacity < *bytes) return fail(MRT_ERR_TOO_LARGE, "copy_wide_nodes: output buffer too small");
    DeviceGuard guard(t->device);
    if (int rc = mrt::wait_refit(t)) return rc;   // a refit in flight writes the array
    MRT_HIP(hipMemcpy(out, t->wide.nodes.get(), (size_t)*bytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}

int mrt_derive_wide_nodes(const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes, int32_t form,
                          void* out, int64_t outCapacity, int64_t* outBytes) {
    if (!nodes || !outBytes || nodeBytes <= 0 || nodeBytes % 64 != 0 || (form != 1 && form != 2) ||
        (woop && (woopBytes <= 0 || woopBytes % 16 != 0)))
        return fail(MRT_ERR_INVALID_ARG, "derive_wide_nodes: bad arguments");
    // the first word of every Woop slot, when the leaf refs can carry counts
    const int64_t slots = woop ? woopBytes / 16 : 0;
    std::vector<int32_t> woopX;
    if (woop && mrt::leaf_counts_fit(slots)) {
        woopX.resize((size_t)slots);
        for (int64_t i = 0; i < slots; i++) woopX[(size_t)i] = static_cast<const int32_t*>(woop)[4 * i];
    }
    const int32_t* wx = woopX.empty() ? nullptr : woopX.data();
    std::vector<uint32_t> wide;
    const auto* n = static_cast<const int32_t*>(nodes);
    if (form == 2) {
        if (!mrt::build_wide4q(n, nodeBytes / 64, &wide, wx, slots))
            return fail(MRT_ERR_INVALID_ARG, "a box has no finite quantization");
    } else {
        wide = mrt::build_wide4(n, nodeBytes / 64, wx, slots);
    }
    *outBytes = (int64_t)wide.size() * 4;
    if (out) {
        if (outCapacity < *outBytes) return fail(MRT_ERR_TOO_LARGE, "derive_wide_nodes: output buffer too small");
        std::memcpy(out, wide.data(), (size_t)*outBytes);
    }
    return MRT_OK;
}

}  // extern "C"
