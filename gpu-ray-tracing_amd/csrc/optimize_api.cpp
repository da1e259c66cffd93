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

// One pass over the levels of plan p, lowest first: a launch per level above kTreeletTailNodes
// records, one workgroup for all smaller ones (level sizes never grow with the height).
int enqueue_treelets(const TreeletArgs& a, const RefitPlan& p, hipStream_t s, int* launches) {
    const int levels = (int)p.levels.size() - 1;
    for (int l = 1; l < levels; l++) {
        const int begin = (int)p.levels[(size_t)l], count = (int)(p.levels[(size_t)l + 1] - begin);
        if (count > kTreeletTailNodes) {
            MRT_HIP(launch_treelet_level(a, p.order.get(), begin, count, s));
            ++*launches;
            continue;
        }
        MRT_HIP(launch_treelet_tail(a, p.order.get(), p.offsets.get(), l, levels, s));
        ++*launches;
        break;
    }
    return MRT_OK;
}

// The passes and the install, the tree already known to be one within the depth limit (first:
// its derivation and plan). From here on the tree is written: an error leaves the tracer unbound.
int run_optimize(mrt_tracer* t, int rounds, DeriveRun& first, RefitPlan& firstPlan, hipStream_t s,
                 std::chrono::steady_clock::time_point t0) {
    const int64_t numNodes = t->nodeBytes / 64;
    mrt_optimize_info info{};
    DeviceBuf<unsigned> counters;
    MRT_HIP(counters.alloc(MRT_OPTIMIZE_MAX_ROUNDS * sizeof(unsigned)));
    MRT_HIP(hipMemsetAsync(counters.get(), 0, MRT_OPTIMIZE_MAX_ROUNDS * sizeof(unsigned), s));
    EventPair ev[MRT_OPTIMIZE_MAX_ROUNDS];

    DeriveRun next;
    RefitPlan nextPlan;
    bool tooDeep = false;
    for (int r = 0; r < rounds; r++) {
        DeriveRun* run = &first;
        RefitPlan* plan = &firstPlan;
        if (r > 0) {
            next = DeriveRun{};
            nextPlan = RefitPlan{};
            int status = kDeriveOk;
            const char* why = nullptr;
            if (int rc = derive_begin(next, t->nodes, numNodes, s)) return rc;
            if (int rc = derive_plan(next, &nextPlan, s, &status, &why)) return rc;
            if (status == kDeriveMalformed) return fail(MRT_ERR_HIP, std::string("optimize: a pass left no tree: ") + why);
            if (status == kDeriveTooDeep) {
                tooDeep = true;
                break;
            }
            run = &next;
            plan = &nextPlan;
        }
        TreeletArgs a{};
        a.nodes = static_cast<uint32_t*>(const_cast<void*>(t->nodes));   // optimize writes the bound nodes (mrt.h)
        a.numNodes = (int)numNodes;
        a.rewritten = counters.get() + r;
        MRT_HIP(ev[r].start.create());
        MRT_HIP(ev[r].stop.create());
        MRT_HIP(hipEventRecord(ev[r].start, s));
        if (int rc = enqueue_treelets(a, *plan, s, &info.launches)) return rc;
        MRT_HIP(hipEventRecord(ev[r].stop, s));
        MRT_HIP(hipStreamSynchronize(s));   // the next derivation reads what this pass wrote; the plan may go
        info.considered[r] = numNodes - plan->levels[1];
        info.scratch_bytes = (int64_t)run->scratchBytes + (int64_t)(MRT_OPTIMIZE_MAX_ROUNDS * sizeof(unsigned));
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

    // The derived data of the new tree, as a device bind makes them on the same buffers.
    const void* nodes = t->nodes;
    const void* woop = t->woop;
    const int32_t* triIndex = t->triIndex;
    const int64_t nodeBytes = t->nodeBytes, woopBytes = t->woopBytes, triIndexBytes = t->triIndexBytes;
    if (!tooDeep) {
        DeriveRun last;
        RefitPlan p;
        int status = kDeriveOk;
        const char* why = nullptr;
        if (int rc = derive_begin(last, nodes, numNodes, s)) return rc;
        if (int rc = derive_plan(last, &p, s, &status, &why)) return rc;
        if (status == kDeriveMalformed) return fail(MRT_ERR_HIP, std::string("optimize: a pass left no tree: ") + why);
        tooDeep = status == kDeriveTooDeep;
        if (!tooDeep) {
            info.levels = (int32_t)p.levels.size() - 1;
            if (int rc = bind_derived(t, last, std::move(p), nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes, s,
                                      true))
                return rc;
        }
    }
    if (tooDeep) {
        if (int rc = bind_locked(t, nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes)) return rc;
        t->lastDerive = mrt_derive_info{};
    }
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
    if (!t->bound) return fail(MRT_ERR_NOT_BOUND, "optimize before bind (no BVH)");
    DeviceGuard guard(t->device);
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = static_cast<hipStream_t>(stream);
    // this handle's traces and refits read the tree and the derived data
    if (int rc = mrt::wait_all_workspaces(t)) return rc;
    if (int rc = mrt::wait_refit(t)) return rc;

    mrt::DeriveRun first;
    mrt::RefitPlan plan;
    int status = mrt::kDeriveOk;
    const char* why = nullptr;
    if (int rc = mrt::derive_begin(first, t->nodes, t->nodeBytes / 64, s)) return rc;
    if (int rc = mrt::derive_plan(first, &plan, s, &status, &why)) return rc;
    if (status == mrt::kDeriveMalformed)
        return fail(MRT_ERR_INVALID_ARG, std::string("optimize: the bound nodes are not a tree: ") + why);
    if (status == mrt::kDeriveTooDeep)
        return fail(MRT_ERR_TOO_LARGE, "optimize: the bound tree has more than MRT_DERIVE_MAX_LEVELS depth levels");
    if (int rc = mrt::run_optimize(t, rounds, first, plan, s, t0)) {
        (void)hipDeviceSynchronize();
        mrt::unbind_locked(t);   // the tree is written in part, or its derived data are not its own
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
