// bind_api.cpp — binding a Compact2 BVH to a tracer and deriving its 4-wide nodes
// (wide_bvh.cpp): mrt_tracer_bind / _unbind / _bind_info / _copy_wide_nodes and the host-only
// mrt_derive_wide_nodes. The library borrows the bound buffers; the wide array is its own.
// Every bind ends here (install), and what a tracer holds of a bound tree is written here only
// (commit; tracer.hpp).
#include <algorithm>
#include <cstring>

#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;

namespace mrt {

namespace {

// The host collapse (bind-time work, synchronous: the Compact2 nodes come to the host, collapse,
// the array goes back) of b in the form cfg.wide `want` asks for into w, its source map in
// w->srcHost. No array for want 0 or a degenerate tree: the binary traversal and its capacity.
int collapse_wide(const BvhBuffers& b, int want, WideArray* w) {
    *w = WideArray{};
    w->builtFor = want;
    if (!want) return MRT_OK;
    std::vector<int32_t> host((size_t)(b.nodeBytes / 4));
    MRT_HIP(hipMemcpy(host.data(), b.nodes, (size_t)b.nodeBytes, hipMemcpyDeviceToHost));
    // The first word of every Woop slot (the terminators): the leaf refs carry counts.
    const int64_t slots = b.woopBytes / 16;
    const bool counts = leaf_counts_fit(slots);
    std::vector<int32_t> woopX;
    if (counts) {
        woopX.resize((size_t)slots);
        MRT_HIP(hipMemcpy2D(woopX.data(), 4, b.woop, 16, 4, (size_t)slots, hipMemcpyDeviceToHost));
    }
    const int32_t* wx = counts ? woopX.data() : nullptr;
    std::vector<uint32_t> wide;
    std::vector<int32_t> src;
    int format = kNodeWide4;
    // The quantized form when asked for and every box quantizes; else the exact one.
    if (want == 2 && build_wide4q(host.data(), b.numNodes(), &wide, wx, slots)) format = kNodeWide4Q;
    else wide = build_wide4(host.data(), b.numNodes(), wx, slots, &src);
    const int nodeWords = format == kNodeWide4 ? 32 : 16;
    const int64_t need = wide_stack_bound(wide.data(), (int64_t)wide.size() / nodeWords, nodeWords);
    if (need + 1 > kMaxWideStack) return MRT_OK;
    const int64_t bytes = (int64_t)wide.size() * 4;
    if (bytes > kMaxBufferBytes) return fail(MRT_ERR_TOO_LARGE, "4-wide node array above the 32-bit range");
    MRT_HIP(w->nodes.alloc((size_t)bytes));
    MRT_HIP(hipMemcpy(w->nodes.get(), wide.data(), (size_t)bytes, hipMemcpyHostToDevice));
    w->bytes = bytes;
    w->format = format;
    w->leafCounts = counts;
    w->stackCap = std::max<int>(kStackCapacity, (int)need + 1);
    w->stackBound = (int)need;
    w->srcHost = std::move(src);
    return MRT_OK;
}

// What of a bind can fail: the wide array, the derivation's report, the commit.
int make_and_commit(mrt_tracer* t, const BvhBuffers& b, Derivation* d, hipStream_t s, unsigned flags,
                    const std::chrono::steady_clock::time_point* since) {
    const auto t0 = since ? *since : std::chrono::steady_clock::now();
    const bool planned = d && !d->tooDeep;
    WideArray w;
    RefitPlan none;
    mrt_derive_info info{};
    if (planned && t->cfg.wide == 1) {
        if (int rc = derive_wide(d->run, b, &w, s)) return rc;
    } else {   // cfg.wide 2 after a derivation too: the quantized form is the host's. Unbound: no array.
        if (int rc = collapse_wide(b, b ? t->cfg.wide : 0, &w)) return rc;
    }
    if (planned) {
        MRT_HIP(hipStreamSynchronize(s));   // the plan's uploads read d->run; the events are complete
        d->plan.built = true;
    }
    if (d)
        if (int rc = derive_report(d->run, planned, planned && t->cfg.wide == 1 && w.nodes, &info)) return rc;
    Install in;
    in.wide = &w;
    in.plan = planned ? &d->plan : &none;
    in.derive = d ? &info : nullptr;
    in.since = b ? &t0 : nullptr;
    in.keepTunes = flags & kKeepTunes;
    return commit(t, b, in);
}

}  // namespace

int commit(mrt_tracer* t, const BvhBuffers& b, const Install& in) {
    WideArray& wide = in.wide ? *in.wide : t->wide;
    int rc = MRT_OK;
    if ((in.plan ? in.plan->built : t->plan.built) && !wide.srcHost.empty()) {
        const size_t bytes = wide.srcHost.size() * 4;
        hipError_t e = wide.src.alloc(bytes);
        if (e == hipSuccess) e = hipMemcpy(wide.src.get(), wide.srcHost.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hipFail(e, "the wide source map's upload");
        else std::vector<int32_t>().swap(wide.srcHost);
    }
    if (!rc && in.wide) rc = wait_all_workspaces(t);
    if (!rc) rc = wait_refit(t);
    if (rc && b) return rc;
    t->bvh = b;
    if (in.wide) t->wide = std::move(*in.wide);
    if (in.plan) t->plan = std::move(*in.plan);
    if (in.since && in.wide) t->bindMs = ms_since(*in.since);
    if (in.derive) {
        t->lastDerive = *in.derive;
        if (in.since) t->lastDerive.wall_ms = ms_since(*in.since);
    }
    if (!in.keepTunes) tune_reset(t);
    return rc;
}

int install(mrt_tracer* t, const BvhBuffers& b, Derivation* d, hipStream_t s, unsigned flags,
            const std::chrono::steady_clock::time_point* since) {
    DeviceGuard guard(t->device);
    const int rc = make_and_commit(t, b, d, s, flags, since);
    if (rc && b && (flags & kUnbindOnError)) (void)unbind_locked(t);
    return rc;
}

int unbind_locked(mrt_tracer* t) { return install(t, BvhBuffers{}, nullptr, nullptr, 0); }

int refresh_wide(mrt_tracer* t, bool afterRefit) {
    DeviceGuard guard(t->device);
    const auto t0 = std::chrono::steady_clock::now();
    const int want = t->bvh ? t->cfg.wide : 0;
    const bool again = afterRefit || want != t->wide.builtFor;
    WideArray w;
    RefitPlan none;
    const int made = again ? collapse_wide(t->bvh, want, &w) : MRT_OK;
    if (made) w = WideArray{};
    Install in;
    in.wide = again ? &w : nullptr;
    in.plan = afterRefit ? nullptr : &none;
    in.since = afterRefit ? nullptr : &t0;
    in.keepTunes = afterRefit;
    const int rc = commit(t, t->bvh, in);
    return made ? made : rc;
}

int check_bind_args(const mrt_tracer* t, const BvhBuffers& b) {
    if (!t || !b.nodes || !b.woop || !b.triIndex) return fail(MRT_ERR_INVALID_ARG, "null BVH buffer");
    if (b.nodeBytes < 64 || b.woopBytes < 16 || b.triIndexBytes < 4 || (b.nodeBytes % 64) || (b.woopBytes % 16) ||
        (b.triIndexBytes % 4))
        return fail(MRT_ERR_INVALID_ARG, "BVH buffer sizes are not Compact2-shaped");
    if (b.nodeBytes > kMaxBufferBytes || b.woopBytes > kMaxBufferBytes)
        return fail(MRT_ERR_TOO_LARGE, "Compact2 buffer above the 32-bit buffer-offset range");
    if (b.triIndexBytes / 4 != b.woopBytes / 16) return fail(MRT_ERR_INVALID_ARG, "triIndex must hold one int per woop float4");
    return MRT_OK;
}

}  // namespace mrt

extern "C" {

int mrt_tracer_bind(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                    const int32_t* triIndex, int64_t triIndexBytes) {
    const mrt::BvhBuffers b{nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes};
    if (int rc = mrt::check_bind_args(t, b)) return rc;
    std::lock_guard<std::mutex> lock(t->mu);
    return mrt::install(t, b, nullptr, nullptr, 0);
}

int mrt_tracer_unbind(mrt_tracer* t) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    std::lock_guard<std::mutex> lock(t->mu);
    return mrt::unbind_locked(t);
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
