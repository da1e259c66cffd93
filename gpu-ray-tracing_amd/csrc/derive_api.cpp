// derive_api.cpp — the refit plan and the exact 4-wide array of a Compact2 tree derived on the
// device: the sequence of wide_kernel.hip's launches (derive / derive_wide, which bind_api.cpp's
// install, build_api.cpp, refit_api.cpp and optimize_api.cpp call too) behind mrt_tracer_bind_device / _derive_info /
// _copy_refit_plan. Host work per call is O(depth levels): one launch per level or per run of
// small levels and pass, one fixed-size summary read back per topology launch, then a few
// summaries and four bytes per level. No node array crosses to the host.
#include <algorithm>
#include <string>

#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;

namespace mrt {

namespace {

int read_summary(DeriveRun& r, int32_t* sum, hipStream_t s) {
    MRT_HIP(hipMemcpyAsync(sum, r.d.summary, wide::kSummaryWords * 4, hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));
    r.readbacks++;
    return MRT_OK;
}

// One pass over the depth levels, shallowest first (dir > 0) or deepest first: a launch per
// level above kDeriveChainNodes nodes, one workgroup for every run of smaller ones.
int run_pass(DeriveRun& r, DeriveStep step, int dir, hipStream_t s) {
    const int levels = r.depthLevels;
    auto count = [&](int l) { return r.depth[(size_t)l + 1] - r.depth[(size_t)l]; };
    for (int done = 0; done < levels;) {
        const int l = dir > 0 ? done : levels - 1 - done;
        if (count(l) > kDeriveChainNodes) {
            MRT_HIP(launch_derive_level(step, r.d, r.depth[(size_t)l], count(l), s));
            done++;
        } else {
            int run = 1;   // levels l, l + dir, ... that fit one workgroup
            while (done + run < levels && count(l + dir * run) <= kDeriveChainNodes) run++;
            const int first = dir > 0 ? l : l - run + 1;
            MRT_HIP(launch_derive_chain(step, r.d, r.x.depthOffsets, first, first + run, dir, s));
            done += run;
        }
        r.launches++;
    }
    return MRT_OK;
}

int derive_begin(DeriveRun& r, const void* nodes, int64_t numNodes, hipStream_t s) {
    if (!nodes || numNodes < 1 || numNodes > ((int64_t)1 << 26)) return fail(MRT_ERR_INVALID_ARG, "derive: no nodes, or more than 2^26");
    size_t bytes = 0, primBytes = 0;
    MRT_HIP(derive_scratch_bytes((int)numNodes, MRT_DERIVE_MAX_LEVELS, &bytes, &primBytes));
    MRT_HIP(r.scratch.alloc(bytes, s));
    for (Event& e : r.ev) MRT_HIP(e.create());
    r.scratchBytes = bytes;
    r.d = wide::Derive{};
    r.d.nodes = static_cast<const int32_t*>(nodes);
    derive_carve(r.d, r.x, (int)numNodes, MRT_DERIVE_MAX_LEVELS, r.scratch.as<void>(), primBytes);
    return MRT_OK;
}

// Fills p (not built) or sets *tooDeep; *why = refit_levels' reason where the nodes are no tree.
int derive_plan(DeriveRun& r, RefitPlan* p, hipStream_t s, bool* tooDeep, const char** why) {
    *tooDeep = false;
    *why = nullptr;
    const int n = r.d.numNodes;
    int32_t sum[wide::kSummaryWords] = {};
    MRT_HIP(hipEventRecord(r.ev[0], s));
    MRT_HIP(launch_derive_init(r.d, r.x, s));
    r.launches++;

    // Topology: breadth first from node 0. Every launch advances by at least one level, so the
    // loop ends after at most MRT_DERIVE_MAX_LEVELS + 1 launches (and a tree has at most n levels).
    int level = 0, begin = 0, end = 1;
    for (int64_t it = 0;; it++) {
        if (it > (int64_t)MRT_DERIVE_MAX_LEVELS + 1 || it > (int64_t)n + 1)
            return fail(MRT_ERR_HIP, "derive: the topology pass did not end");
        const bool chain = end - begin <= kDeriveChainNodes;
        if (!chain && level >= MRT_DERIVE_MAX_LEVELS) {
            *tooDeep = true;
            return MRT_OK;
        }
        if (chain) MRT_HIP(launch_derive_expand_chain(r.d, r.x.depthOffsets, level, begin, end, MRT_DERIVE_MAX_LEVELS, s));
        else MRT_HIP(launch_derive_expand(r.d, r.x.depthOffsets, level, begin, end - begin, s));
        r.launches++;
        if (int rc = read_summary(r, sum, s)) return rc;
        if (sum[wide::kError]) break;
        const int reached = std::min(std::max(sum[wide::kReached], end), n);
        if (chain) {
            const int l = sum[wide::kNextLevel], b = sum[wide::kFrontBegin], e = sum[wide::kFrontEnd];
            if (l < level || l > MRT_DERIVE_MAX_LEVELS || b < begin || e < b || e > n)
                return fail(MRT_ERR_HIP, "derive: the topology pass reported an impossible frontier");
            level = l;
            begin = b;
            end = e;
            if (begin == end) break;   // the last level's end is written: done
            if (level >= MRT_DERIVE_MAX_LEVELS) {
                *tooDeep = true;
                return MRT_OK;
            }
        } else {
            begin = end;
            end = reached;
            level++;
        }
    }
    if ((*why = wide::error_text(sum[wide::kError], sum[wide::kReached], n))) return MRT_OK;
    r.depthLevels = level;
    r.depth.assign((size_t)level + 1, 0);
    MRT_HIP(hipMemcpyAsync(r.depth.data(), r.x.depthOffsets, r.depth.size() * 4, hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));
    r.readbacks++;
    for (int l = 0; l < level; l++)
        if (r.depth[(size_t)l] < 0 || r.depth[(size_t)l + 1] <= r.depth[(size_t)l]) return fail(MRT_ERR_HIP, "derive: depth levels out of order");
    if (level < 1 || r.depth[0] != 0 || r.depth[(size_t)level] != n) return fail(MRT_ERR_HIP, "derive: depth levels do not cover the nodes");

    // Heights, deepest level first; then the nodes by (height, index).
    if (int rc = run_pass(r, kStepHeight, -1, s)) return rc;
    int32_t top = -1;   // node 0's height is the tree's
    MRT_HIP(hipMemcpyAsync(&top, r.d.height, 4, hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));
    r.readbacks++;
    if (top < 0 || top >= level) return fail(MRT_ERR_HIP, "derive: a height above the depth");
    r.offsets32.assign((size_t)top + 2, -1);
    MRT_HIP(p->order.alloc((size_t)n * 4));
    MRT_HIP(p->offsets.alloc(r.offsets32.size() * 4));
    MRT_HIP(p->valid.alloc((size_t)n * 2));
    MRT_HIP(p->skipped.alloc(sizeof(unsigned long long)));
    MRT_HIP(hipMemsetAsync(p->skipped.get(), 0, sizeof(unsigned long long), s));
    MRT_HIP(launch_derive_sort(r.d, r.x, p->order.get(), p->offsets.get(), top + 1, s));
    r.launches += 2;
    MRT_HIP(hipEventRecord(r.ev[1], s));
    MRT_HIP(hipMemcpyAsync(r.offsets32.data(), p->offsets.get(), r.offsets32.size() * 4, hipMemcpyDeviceToHost, s));
    MRT_HIP(hipStreamSynchronize(s));
    r.readbacks++;
    for (size_t h = 0; h + 1 < r.offsets32.size(); h++)
        if (r.offsets32[h] < 0 || r.offsets32[h + 1] <= r.offsets32[h]) return fail(MRT_ERR_HIP, "derive: height levels out of order");
    if (r.offsets32.front() != 0 || r.offsets32.back() != n) return fail(MRT_ERR_HIP, "derive: height levels do not cover the nodes");
    p->levels.assign(r.offsets32.begin(), r.offsets32.end());
    p->bytes = (int64_t)n * 4 + (int64_t)r.offsets32.size() * 4 + (int64_t)n * 2 + 8;
    return MRT_OK;
}

}  // namespace

int derive(Derivation& d, const void* nodes, int64_t numNodes, hipStream_t s, int code, const char* prefix) {
    const char* why = nullptr;
    if (int rc = derive_begin(d.run, nodes, numNodes, s)) return rc;
    if (int rc = derive_plan(d.run, &d.plan, s, &d.tooDeep, &why)) return rc;
    return why ? fail(code, std::string(prefix) + why) : MRT_OK;
}

// The exact 4-wide array of r's tree (its plan derived, its boxes final) into w; no array where
// the stack bound is above the limit: the binary traversal stays.
int derive_wide(DeriveRun& r, const BvhBuffers& b, WideArray* w, hipStream_t s) {
    *w = WideArray{};
    const int n = r.d.numNodes;
    int32_t sum[wide::kSummaryWords] = {};
    int32_t numWide = 0;
    MRT_HIP(hipEventRecord(r.ev[2], s));
    if (int rc = run_pass(r, kStepFlag, +1, s)) return rc;
    if (int rc = run_pass(r, kStepSize, -1, s)) return rc;
    MRT_HIP(hipMemcpyAsync(&numWide, r.d.size, 4, hipMemcpyDeviceToHost, s));
    if (int rc = read_summary(r, sum, s)) return rc;
    if (sum[wide::kError] || numWide < 1 || numWide > n) return fail(MRT_ERR_HIP, "derive: the collapse left the tree");
    w->bytes = (int64_t)numWide * 128;
    if (w->bytes > kMaxBufferBytes) return fail(MRT_ERR_TOO_LARGE, "4-wide node array above the 32-bit range");
    if (int rc = run_pass(r, kStepIndex, +1, s)) return rc;
    MRT_HIP(w->nodes.alloc((size_t)w->bytes));
    MRT_HIP(w->src.alloc((size_t)numWide * 16));
    const int64_t slots = b.woopBytes / 16;
    w->leafCounts = leaf_counts_fit(slots);
    r.d.woopX = w->leafCounts ? static_cast<const int32_t*>(b.woop) : nullptr;
    r.d.woopStride = 4;
    r.d.woopSlots = slots;
    r.d.wideOut = w->nodes.get();
    r.d.srcOut = w->src.get();
    r.d.numWide = numWide;
    MRT_HIP(hipEventRecord(r.ev[3], s));
    MRT_HIP(launch_derive_emit(r.d, s));
    r.launches++;
    MRT_HIP(hipEventRecord(r.ev[4], s));
    if (int rc = read_summary(r, sum, s)) return rc;
    const int64_t need = sum[wide::kStackBound];
    if (need < 0 || need + 1 > kMaxWideStack) *w = WideArray{};
    else {
        w->format = kNodeWide4;
        w->stackCap = std::max<int>(kStackCapacity, (int)need + 1);
        w->stackBound = (int)need;
    }
    w->builtFor = 1;
    return MRT_OK;
}

int derive_report(const DeriveRun& r, bool plan, bool wide, mrt_derive_info* out) {
    mrt_derive_info info{};
    info.on_device_plan = plan;
    info.on_device_wide = wide;
    info.levels = plan ? (int32_t)r.offsets32.size() - 1 : 0;
    info.depth_levels = r.depthLevels;
    info.wide_nodes = wide ? r.d.numWide : 0;
    info.launches = r.launches;
    info.readbacks = r.readbacks;
    if (plan) MRT_HIP(hipEventElapsedTime(&info.topo_ms, r.ev[0], r.ev[1]));
    if (wide) {
        MRT_HIP(hipEventElapsedTime(&info.collapse_ms, r.ev[2], r.ev[3]));
        MRT_HIP(hipEventElapsedTime(&info.emit_ms, r.ev[3], r.ev[4]));
    }
    info.scratch_bytes = (int64_t)r.scratchBytes;
    *out = info;
    return MRT_OK;
}

}  // namespace mrt

extern "C" {

int mrt_tracer_bind_device(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                           const int32_t* triIndex, int64_t triIndexBytes, void* stream) {
    const mrt::BvhBuffers b{nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes};
    if (int rc = mrt::check_bind_args(t, b)) return rc;
    std::lock_guard<std::mutex> lock(t->mu);
    DeviceGuard guard(t->device);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = static_cast<hipStream_t>(stream);
    mrt::Derivation d;
    if (int rc = mrt::derive(d, b.nodes, b.numNodes(), s, MRT_ERR_INVALID_ARG, "bind_device: the nodes are not a tree: ")) {
        (void)mrt::unbind_locked(t);   // mrt.h: a refused tree leaves the tracer unbound
        return rc;
    }
    // too deep: the host path, and the info says so
    return mrt::install(t, b, &d, s, mrt::kUnbindOnError, &t0);
}

int mrt_tracer_derive_info(mrt_tracer* t, mrt_derive_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    *info = t->lastDerive;
    return MRT_OK;
}

int mrt_tracer_copy_refit_plan(mrt_tracer* t, int32_t* order, int64_t* levelOffsets, int32_t levelCapacity,
                               int32_t* numLevels, int32_t* wideSrc, int64_t wideSrcCapacity, int64_t* numWideSrc) {
    if (!t || !numLevels || levelCapacity < 0 || wideSrcCapacity < 0)
        return fail(MRT_ERR_INVALID_ARG, "copy_refit_plan: bad arguments");
    std::lock_guard<std::mutex> lock(t->mu);
    const mrt::RefitPlan& p = t->plan;
    *numLevels = 0;
    if (numWideSrc) *numWideSrc = 0;
    if (!p.built) return MRT_OK;
    DeviceGuard guard(t->device);
    if (int rc = mrt::wait_refit(t)) return rc;
    *numLevels = (int32_t)p.levels.size() - 1;
    if (order) MRT_HIP(hipMemcpy(order, p.order.get(), (size_t)p.levels.back() * 4, hipMemcpyDeviceToHost));
    if (levelOffsets) {
        if (levelCapacity < (int32_t)p.levels.size()) return fail(MRT_ERR_TOO_LARGE, "copy_refit_plan: levelOffsets too small");
        std::vector<int32_t> dev(p.levels.size());   // the device's copy, not the host's
        MRT_HIP(hipMemcpy(dev.data(), p.offsets.get(), dev.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < dev.size(); i++) levelOffsets[i] = dev[i];
    }
    const int32_t* src = t->wide.src.get();
    if (numWideSrc && src) {
        *numWideSrc = t->wide.bytes / 128 * 4;
        if (wideSrc) {
            if (wideSrcCapacity < *numWideSrc) return fail(MRT_ERR_TOO_LARGE, "copy_refit_plan: wideSrc too small");
            MRT_HIP(hipMemcpy(wideSrc, src, (size_t)*numWideSrc * 4, hipMemcpyDeviceToHost));
        }
    }
    return MRT_OK;
}

}  // extern "C"
