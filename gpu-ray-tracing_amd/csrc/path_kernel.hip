// path_kernel.hip — a path frame's kernels on the device (gfx950): one vertex of every live path
// with stable compaction of the survivors, the accumulation of a traced shadow batch, and the
// resolve of a batch's paths into pixels (path_kernel.hpp). The C-ABI that calls them is
// path_api.cpp.
//
//   count_kernel       survivors of each 256-slot workgroup, from the result ids (4 bytes per slot;
//                      in-place mode also reads the slot's task)
//   scan_kernel        one workgroup: the exclusive prefix sum of those counts, 1024 per round,
//                      and the total into the device live count
//   extend_kernel      path_common.hpp's vertex step, one lane per slot; a survivor's records go to
//                      slot  base[workgroup] + waves before it (LDS) + set ballot bits below the lane
//                      which is the number of survivors before it: the order is stable and the same
//                      from run to run
//   accumulate_kernel  radiance[task] += pending where the shadow ray reached the light
//   resolve_kernel     one lane per primary ray of the batch
//
// No workgroup waits on another: the three compaction steps are three launches in stream order.
// No float atomics: a path's radiance is added to by the one lane that holds the path, vertex
// after vertex. The per-path arithmetic is csrc/path_common.hpp, the same code the host runs
// (csrc/host/path.cpp); this file is built without denormal flushing (Makefile), so the bits are
// the host's. Rays move as two 16-byte halves, states and pending contributions as one.
#include "path_kernel.hpp"

#include "path_limits.hpp"
#include "record_device.hpp"

namespace mrt {
namespace {

using namespace path;

__device__ inline State load_state(const State* states, int64_t at) {
    const int4 v = reinterpret_cast<const int4*>(states)[at];
    return State{__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), v.w};
}

__device__ inline void store_state(State* states, int64_t at, const State& s) {
    reinterpret_cast<int4*>(states)[at] = make_int4(__float_as_int(s.tr), __float_as_int(s.tg), __float_as_int(s.tb), s.task);
}

__device__ inline bool in_tree(int32_t id, int64_t numTris) { return id >= 0 && (int64_t)id < numTris; }

struct ExtendArgs : PathExtendLaunch {};

__global__ __launch_bounds__(kThreads) void count_kernel(ExtendArgs a) {
    __shared__ int waveCount[kWaves];
    const int slot = (int)(blockIdx.x * kThreads + threadIdx.x);
    bool survivor = false;
    if (slot < a.numSlots) {
        const int64_t at = a.p.vertex == 0 ? slot / a.p.numSamples : slot;
        survivor = in_tree(a.inResults[2 * at].x, a.p.numTris);
        if (!a.compact && a.p.vertex != 0) survivor = survivor && owns(load_state(a.inState, slot).task, a.numPaths);
    }
    const unsigned long long m = __ballot(survivor);
    if ((threadIdx.x & 63) == 0) waveCount[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kWaves; w++) c += waveCount[w];
        a.counts[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(kScanThreads) void scan_kernel(int32_t* counts, int numCounts, int32_t* liveCount) {
    constexpr int kScanWaves = kScanThreads / 64;
    __shared__ int waveTotal[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int first = 0; first < numCounts; first += kScanThreads) {   // uniform: every thread runs every round
        const int i = first + (int)threadIdx.x;
        const int v = i < numCounts ? counts[i] : 0;
        int incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) waveTotal[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < kScanWaves; w++) {
            const int t = waveTotal[w];
            if (w < wave) before += t;
            all += t;
        }
        if (i < numCounts) counts[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();   // waveTotal is rewritten by the next round
    }
    if (threadIdx.x == 0) *liveCount = carry;
}

__global__ __launch_bounds__(kThreads) void extend_kernel(ExtendArgs a) {
    __shared__ int waveCount[kWaves];
    const int slot = (int)(blockIdx.x * kThreads + threadIdx.x);
    const bool valid = slot < a.numSlots;
    bool live = false;
    Step st;
    st.survivor = st.escaped = false;
    if (valid) {
        State state = first_state(slot);
        int64_t at = slot;
        if (a.p.vertex == 0) {
            at = slot / a.p.numSamples;
            live = true;
        } else {
            state = load_state(a.inState, slot);
            live = owns(state.task, a.numPaths);
        }
        if (live) {
            const int2 res = a.inResults[2 * at];
            extend(a.p, load_ray(a.inRays, at), res.x, __int_as_float(res.y), state, st);
        }
    }
    const bool survivor = live && st.survivor;
    const unsigned long long m = __ballot(survivor);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) waveCount[wave] = __popcll(m);
    __syncthreads();
    int64_t dest = slot;
    if (a.compact) {
        int base = a.counts[blockIdx.x];
        for (int w = 0; w < wave; w++) base += waveCount[w];
        dest = base + below;   // < the scan's total <= numSlots
    }
    if (survivor) {
        store_ray(a.outShadow, dest, st.shadow);
        a.outPending[dest] = make_float4(st.pending[0], st.pending[1], st.pending[2], 0.0f);
        if (a.p.vertex < a.p.depth) store_ray(a.outRays, dest, st.bounce);
        store_state(a.outState, dest, st.state);
    } else if (valid && !a.compact) {
        store_ray(a.outShadow, slot, dead_ray());
        a.outPending[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.p.vertex < a.p.depth) store_ray(a.outRays, slot, dead_ray());
        store_state(a.outState, slot, dead_state());
    }
    if (live && st.escaped) {
        float4 r = a.radiance[st.task];
        r.x += st.add[0];
        r.y += st.add[1];
        r.z += st.add[2];
        a.radiance[st.task] = r;
    }
}

struct AccumulateArgs : PathAccumulateLaunch {};

__global__ __launch_bounds__(kThreads) void accumulate_kernel(AccumulateArgs a) {
    const int slot = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (slot >= a.numSlots) return;
    const int32_t task = load_state(a.state, slot).task;
    if (!owns(task, a.numPaths) || a.shadowResults[slot].x != -1) return;
    const float4 p = a.pending[slot];
    float4 r = a.radiance[task];
    r.x += p.x;
    r.y += p.y;
    r.z += p.z;
    a.radiance[task] = r;
}

struct ResolveArgs : PathResolveLaunch {};

__global__ __launch_bounds__(kThreads) void resolve_kernel(ResolveArgs a) {
    const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= a.numPrimary) return;
    const int slot = a.firstPrimary + i;
    const int pixel = a.primarySlotToId[slot];
    float v[4];
    if (a.primaryResults[slot].x == -1) {
        background(v);
    } else {
        resolve_one(reinterpret_cast<const float*>(a.radiance) + 4 * (int64_t)i * a.numSamples, a.numSamples, v);
    }
    a.pixels[pixel] = light::to_abgr(v);
    if (a.image) a.image[pixel] = make_float4(v[0], v[1], v[2], v[3]);
}

template <class K, class A>
hipError_t launch(K kernel, int grid, int threads, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_path_count(const PathExtendLaunch& a, int grid, hipStream_t s) {
    return launch(count_kernel, grid, kThreads, s, ExtendArgs{a});
}

hipError_t launch_path_scan(int32_t* counts, int numCounts, int32_t* liveCount, hipStream_t s) {
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3((unsigned)kScanThreads), 0, s, counts, numCounts, liveCount);
    return hipGetLastError();
}

hipError_t launch_path_extend(const PathExtendLaunch& a, int grid, hipStream_t s) {
    return launch(extend_kernel, grid, kThreads, s, ExtendArgs{a});
}

hipError_t launch_path_accumulate(const PathAccumulateLaunch& a, int grid, hipStream_t s) {
    return launch(accumulate_kernel, grid, kThreads, s, AccumulateArgs{a});
}

hipError_t launch_path_resolve(const PathResolveLaunch& a, int grid, hipStream_t s) {
    return launch(resolve_kernel, grid, kThreads, s, ResolveArgs{a});
}

}  // namespace mrt
