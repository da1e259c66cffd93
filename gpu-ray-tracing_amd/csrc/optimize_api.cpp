// optimize_api.cpp — re-optimising the bound BVH on the device by treelet restructuring: per pass
// the level plan (derive_api.cpp's derivation, which validates the tree) and the launches
// (treelet_kernel.hip), then the derived data installed as a device bind does, behind
// mrt_tracer_optimize / _optimize_info.
#include <string>

#include "tracer.hpp"
#include "treelet_kernel.hpp"

using mrt::DeviceGuard;
using mrt::fail;

namespace mrt {

namespace {

const char* const kPassPrefix = "optimize: a pass left no tree: ";

// One pass over the levels of plan p, lowest first (walk_levels above kTreeletTailNodes records).
int enqueue_treelets(const TreeletArgs& a, const RefitPlan& p, hipStream_t s, int* launches) {
    return walk_levels(
        p.levels, kTreeletTailNodes, launches,
        [&](int begin, int count) { return launch_treelet_level(a, p.order.get(), begin, count, s); },
        [&](int first, int levels) { return launch_treelet_tail(a, p.order.get(), p.offsets.get(), first, levels, s); });
}

// The passes and the install, the tree already known to be one within the depth limit (first:
// its derivation). From here on the tree is written: an error leaves the tracer unbound.
int run_optimize(mrt_tracer* t, int rounds, Derivation& first, hipStream_t s,
                 std::chrono::steady_clock::time_point t0) {
    const BvhBuffers b = t->bvh;
    const int64_t numNodes = b.numNodes();
    mrt_optimize_info info{};
    DeviceBuf<unsigned> counters;
    MRT_HIP(counters.alloc(MRT_OPTIMIZE_MAX_ROUNDS * sizeof(unsigned)));
    MRT_HIP(hipMemsetAsync(counters.get(), 0, MRT_OPTIMIZE_MAX_ROUNDS * sizeof(unsigned), s));
    EventPair ev[MRT_OPTIMIZE_MAX_ROUNDS];

    Derivation next;
    for (int r = 0; r < rounds; r++) {
        Derivation* d = &first;
        if (r > 0) {
            next = Derivation{};
            if (int rc = derive(next, b.nodes, numNodes, s, MRT_ERR_HIP, kPassPrefix)) return rc;
            if (next.tooDeep) break;
            d = &next;
        }
        TreeletArgs a{};
        a.nodes = static_cast<uint32_t*>(const_cast<void*>(b.nodes));   // optimize writes the bound nodes (mrt.h)
        a.numNodes = (int)numNodes;
        a.rewritten = counters.get() + r;
        MRT_HIP(ev[r].start.create());
        MRT_HIP(ev[r].stop.create());
        MRT_HIP(hipEventRecord(ev[r].start, s));
        if (int rc = enqueue_treelets(a, d->plan, s, &info.launches)) return rc;
        MRT_HIP(hipEventRecord(ev[r].stop, s));
        MRT_HIP(hipStreamSynchronize(s));   // the next derivation reads what this pass wrote; the plan may go
        info.considered[r] = numNodes - d->plan.levels[1];
        info.scratch_bytes = (int64_t)d->run.scratchBytes + (int64_t)(MRT_OPTIMIZE_MAX_ROUNDS * sizeof(unsigned));
        info.rounds = r + 1;
    }
    unsigned rewritten[MRT_OPTIMIZE_MAX_ROUNDS] = {};
    MRT_HIP(hipMemcpy(rewritten, counters.get(), sizeof rewritten, hipMemcpyDeviceToHost));
    for (int r = 0; r < info.rounds; r++) {
        info.rewritten[r] = rewritten[r];
        float ms = 0.0f;
        MRT_HIP(hipEventElapsedTime(&ms, ev[r].start, ev[r].stop));
        info.device_ms += ms;
    }

    // The derived data of the new tree, as a device bind makes them on the same buffers. A tree
    // too deep after a pass (none observed) goes through the host path, which forgets the schedules.
    Derivation last;
    Derivation* fin = &next;
    if (!next.tooDeep) {
        if (int rc = derive(last, b.nodes, numNodes, s, MRT_ERR_HIP, kPassPrefix)) return rc;
        fin = &last;
    }
    if (!fin->tooDeep) info.levels = (int32_t)fin->plan.levels.size() - 1;
    if (int rc = install(t, b, fin, s, fin->tooDeep ? 0 : kKeepTunes)) return rc;
    info.wall_ms = ms_since(t0);
    t->lastOptimize = info;
    return MRT_OK;
}

}  // namespace

}  // namespace mrt

extern "C" {

int mrt_tracer_optimize(mrt_tracer* t, const mrt_optimize_params* params, void* stream) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    const int rounds = params && params->rounds ? params->rounds : 1;
    if (rounds < 1 || rounds > MRT_OPTIMIZE_MAX_ROUNDS) return fail(MRT_ERR_INVALID_ARG, "optimize: rounds outside 0..8");
    std::lock_guard<std::mutex> lock(t->mu);
    if (!t->bvh) return fail(MRT_ERR_NOT_BOUND, "optimize before bind (no BVH)");
    DeviceGuard guard(t->device);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = static_cast<hipStream_t>(stream);
    // this handle's traces and refits read the tree and the derived data
    if (int rc = mrt::wait_all_workspaces(t)) return rc;
    if (int rc = mrt::wait_refit(t)) return rc;

    mrt::Derivation first;
    if (int rc = mrt::derive(first, t->bvh.nodes, t->bvh.numNodes(), s, MRT_ERR_INVALID_ARG,
                             "optimize: the bound nodes are not a tree: "))
        return rc;
    if (first.tooDeep)
        return fail(MRT_ERR_TOO_LARGE, "optimize: the bound tree has more than MRT_DERIVE_MAX_LEVELS depth levels");
    if (int rc = mrt::run_optimize(t, rounds, first, s, t0)) {
        (void)hipDeviceSynchronize();
        (void)mrt::unbind_locked(t);   // the tree is written in part, or its derived data are not its own
        return rc;
    }
    return MRT_OK;
}

int mrt_tracer_optimize_info(mrt_tracer* t, mrt_optimize_info* info) {
    if (!t || !info) return fail(MRT_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lock(t->mu);
    *info = t->lastOptimize;
    return MRT_OK;
}

}  // extern "C"
