// treelet_kernel.hip — gfx950 kernels that restructure the treelets of a bound Compact2 tree in
// place (mrt_tracer_optimize; the CPU statement is csrc/host/treelet.cpp, the arithmetic
// treelet_common.hpp's on both sides).
//
// A round is a short chain of launches, lowest height level first (level 0 has nothing to do):
//   treelet_level  one launch per level of more than kTreeletTailNodes records, one wave per
//                  record: lane 0 forms the treelet into LDS, the 64 lanes take the up to 127
//                  subset areas two each, the dynamic programme runs in seven steps by subset
//                  size with each subset's partitions enumerated by ONE lane in the header's
//                  order (so its tie rule needs no parallel minimum), lane 0 emits
//   treelet_tail   every remaining level in ONE workgroup of 16 waves, a barrier between levels
//                  (level sizes never grow with the height)
// Records of equal height have disjoint subtrees and a treelet's records all lie in its root's
// subtree, so no wave touches another's records inside a level; a wave reads only bytes written
// by EARLIER launches, or (treelet_tail) by its own workgroup before a barrier. No workgroup
// waits on another.
//
// This file is built WITHOUT -fgpu-flush-denormals-to-zero (Makefile), with -ffp-contract=off:
// every area and sum is the IEEE float32 the host computes, so every comparison falls as it
// does there and the bytes written are the host's. Every ref read from memory is range-checked
// before it is followed (treelet::inner_ref), every root index before it is used.
#include "treelet_kernel.hpp"
#include "treelet_common.hpp"

namespace mrt {

namespace {

constexpr int kWave = 64;
constexpr int kLevelWaves = 4;
constexpr int kTailWaves = 16;

struct WaveState {
    treelet::Treelet t;
    treelet::Dp d;
    int go;
};

// One treelet per wave; root < 0: nothing to do. Every wave of the workgroup passes the same
// number of barriers whatever its treelet is.
__device__ __forceinline__ void wave_treelet(const TreeletArgs& a, int root, WaveState& w, int lane) {
    if (lane == 0) {
        w.go = 0;
        if (root >= 0 && root < a.numNodes) {
            treelet::form(a.nodes, a.numNodes, root, w.t);
            w.go = treelet::leaves_ok(w.t) ? 1 : 0;
        }
    }
    __syncthreads();
    const bool go = w.go != 0;
    const int full = go ? (1 << w.t.n) - 1 : 0;
    bool bad = false;
    for (int S = lane; S <= full; S += kWave) {
        if (!S) continue;
        const float ar = treelet::subset_area(w.t, S);
        w.d.a[S] = ar;
        bad |= !treelet::finite(ar);
    }
    const bool ok = go && __ballot(bad) == 0;   // the whole wave, also where go is false
    __syncthreads();
    for (int size = 1; size <= treelet::kMaxLeaves; size++) {
        if (ok)
            for (int S = lane; S <= full; S += kWave)
                if (S && __popc(S) == size) treelet::solve_subset(w.d, S, full);
        __syncthreads();
    }
    if (ok && lane == 0 && treelet::worth_it(w.t, w.d) && treelet::emit(a.nodes, root, w.t, w.d))
        atomicAdd(a.rewritten, 1u);
    __syncthreads();   // this workgroup's stores before its next loads; w is free again
}

__global__ __launch_bounds__(kLevelWaves* kWave) void treelet_level_kernel(TreeletArgs a, const int32_t* order, int begin,
                                                                          int count) {
    __shared__ WaveState state[kLevelWaves];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int64_t i = (int64_t)blockIdx.x * kLevelWaves + wave;
    wave_treelet(a, i < count ? order[begin + i] : -1, state[wave], lane);
}

__global__ __launch_bounds__(kTailWaves* kWave) void treelet_tail_kernel(TreeletArgs a, const int32_t* order,
                                                                        const int32_t* offsets, int firstLevel,
                                                                        int numLevels) {
    __shared__ WaveState state[kTailWaves];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int l = firstLevel; l < numLevels; l++) {
        const int begin = offsets[l], end = offsets[l + 1];
        if (begin < 0 || end > a.numNodes) return;   // the same for every thread
        for (int base = begin; base < end; base += kTailWaves)
            wave_treelet(a, base + wave < end ? order[base + wave] : -1, state[wave], lane);
    }
}

}  // namespace

hipError_t launch_treelet_level(const TreeletArgs& a, const int32_t* order, int begin, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int blocks = (count + kLevelWaves - 1) / kLevelWaves;
    hipLaunchKernelGGL(treelet_level_kernel, dim3(blocks), dim3(kLevelWaves * kWave), 0, s, a, order, begin, count);
    return hipGetLastError();
}

hipError_t launch_treelet_tail(const TreeletArgs& a, const int32_t* order, const int32_t* offsets, int firstLevel,
                               int numLevels, hipStream_t s) {
    if (firstLevel >= numLevels) return hipSuccess;
    hipLaunchKernelGGL(treelet_tail_kernel, dim3(1), dim3(kTailWaves * kWave), 0, s, a, order, offsets, firstLevel,
                       numLevels);
    return hipGetLastError();
}

}  // namespace mrt
