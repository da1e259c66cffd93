// wide_kernel.hip — gfx950 kernels that derive, from a Compact2 tree on the device, what a bind
// and the first refit used to compute on the host: the refit plan (the nodes by height level)
// and the exact 4-wide array with its source map and stack bound (wide_bvh.cpp's bytes). The
// per-node arithmetic is wide_common.hpp's on both sides; derive_api.cpp sequences the launches.
//
// Every pass goes depth level by depth level, one launch per level:
//   expand   (down)  topology: a node claims its inner children (an atomic on `visited`) and
//                    appends them to byDepth; a ref outside the array or a node claimed twice
//                    sets an error bit and is not followed, so a cycle or a DAG ends
//   height   (up)    0 for two leaf children, else 1 + the highest inner child
//   (rocPRIM)        stable radix sort of (height, node index): the plan's order; the level
//                    starts are where the sorted height changes
//   flag     (down)  a wide root collapses its subtree's top and flags its inner wide children
//                    as roots (they lie 1 to 3 levels deeper)
//   size     (up)    wide nodes below a wide root, itself included
//   index    (down)  depth-first numbers and the stack entries on the way (the stack bound)
//   emit     (one launch over all nodes) a wide root writes its 128-byte node and source slots
// A thread reads only what EARLIER launches wrote, or (the chained launches) what its own
// workgroup wrote before a barrier: consecutive levels of at most kDeriveChainNodes nodes run
// in one workgroup. No workgroup waits on or reads another's output inside a launch (the
// per-XCD L2s and per-CU L1s make such hand-offs a hazard, refit_kernel.hip); the claims, the
// counters and the error bits are atomics, which the L2 serves. The two counters every node
// would hit (nodes reached, the stack bound) take one atomic per wave: one per node serialised
// 2.4 M adds on one address, 11 of hairball's 15 ms.
//
// Built WITHOUT -fgpu-flush-denormals-to-zero and with -ffp-contract=off (Makefile): the
// collapse compares double areas of float differences, and a flushed denormal or a contracted
// fma would pick other children than the host does.
//
// Every index read from memory is range-checked before it addresses anything (the steps of
// wide_common.hpp check node indices, refs, wide numbers and Woop slots).
#include "wide_kernel.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace mrt {

namespace {

constexpr int kBlock = 256;

// Positions in a list for `cnt` (0..2) new entries of every lane: one atomic per wave. Every
// lane of the wave calls it (the callers keep their control flow uniform up to here).
__device__ __forceinline__ int wave_alloc(int32_t* counter, int cnt) {
    const unsigned long long b1 = __ballot(cnt >= 1), b2 = __ballot(cnt >= 2);
    const int total = __popcll(b1) + __popcll(b2);
    const unsigned lane = __lane_id();
    const unsigned long long lower = lane ? (~0ull >> (64 - lane)) : 0ull;
    int base = 0;
    if (lane == 0 && total) base = atomicAdd(counter, total);
    return __shfl(base, 0) + __popcll(b1 & lower) + __popcll(b2 & lower);
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// Node n's step; n < 0: this lane has no node (it still takes part in the wave's counters).
template <int STEP>
__device__ __forceinline__ void run_step(const wide::Derive& d, int32_t n) {
    if (STEP == kStepExpand) {
        int32_t kid[2] = {0, 0};
        const int cnt = n >= 0 ? wide::step_claim(d, n, kid) : 0;
        const int pos = wave_alloc(d.summary + wide::kReached, cnt);
        for (int k = 0; k < cnt; k++)
            if ((uint32_t)(pos + k) < (uint32_t)d.numNodes) d.byDepth[pos + k] = kid[k];
    }
    if (STEP == kStepHeight && n >= 0) wide::step_height(d, n);
    if (STEP == kStepFlag && n >= 0) wide::step_flag(d, n);
    if (STEP == kStepSize && n >= 0) wide::step_size(d, n);
    if (STEP == kStepIndex) {
        const int below = wave_max(n >= 0 ? wide::step_index(d, n) : 0);
        if (__lane_id() == 0 && below > 0) atomicMax(d.summary + wide::kStackBound, below);
    }
}

__global__ __launch_bounds__(kBlock) void derive_init_kernel(wide::Derive d, int32_t* ids) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < wide::kSummaryWords) d.summary[i] = i == wide::kReached ? 1 : 0;
    if (i >= d.numNodes) return;
    d.visited[i] = i == 0;
    d.size[i] = i == 0;
    ids[i] = i;
    if (i == 0) d.byDepth[0] = d.index[0] = d.entries[0] = 0;
}

template <int STEP>
__global__ __launch_bounds__(kBlock) void derive_level_kernel(wide::Derive d, int begin, int count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    run_step<STEP>(d, i < count ? d.byDepth[begin + i] : -1);
}

__global__ __launch_bounds__(kBlock) void derive_expand_kernel(wide::Derive d, int32_t* depthOffsets, int level,
                                                               int begin, int count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) depthOffsets[level] = begin;
    run_step<kStepExpand>(d, i < count ? d.byDepth[begin + i] : -1);
}

template <int STEP>
__global__ __launch_bounds__(kDeriveChainNodes) void derive_chain_kernel(wide::Derive d, const int32_t* depthOffsets,
                                                                         int first, int last, int dir) {
    for (int k = 0; k < last - first; k++) {
        const int l = dir > 0 ? first + k : last - 1 - k;
        const int end = min(depthOffsets[l + 1], d.numNodes);
        for (int base = max(depthOffsets[l], 0); base < end; base += kDeriveChainNodes) {   // uniform trip count
            const int i = base + (int)threadIdx.x;
            run_step<STEP>(d, i < end ? d.byDepth[i] : -1);
        }
        __syncthreads();   // this workgroup's stores of level l before its loads of the next one
    }
}

__global__ __launch_bounds__(kDeriveChainNodes) void derive_expand_chain_kernel(wide::Derive d, int32_t* depthOffsets,
                                                                                int level, int begin, int end,
                                                                                int maxLevels) {
    // begin, end and level are the same in every thread: `reached` is read between two barriers
    while (true) {
        const int count = end - begin;
        if (threadIdx.x == 0 && level <= maxLevels) depthOffsets[level] = begin;
        if (count <= 0 || count > kDeriveChainNodes || level >= maxLevels) break;
        const int i = begin + (int)threadIdx.x;   // at most one node per thread
        run_step<kStepExpand>(d, i < end ? d.byDepth[i] : -1);
        __syncthreads();   // every claim of this level is counted
        const int reached =
            min(__hip_atomic_load(d.summary + wide::kReached, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), d.numNodes);
        __syncthreads();   // and read by all before the next level counts on
        begin = end;
        end = max(reached, end);
        level++;
    }
    if (threadIdx.x == 0) {
        d.summary[wide::kNextLevel] = level;
        d.summary[wide::kFrontBegin] = begin;
        d.summary[wide::kFrontEnd] = end;
    }
}

// The level starts from the sorted heights: offsets[h] = the first position of height h (every
// height 0 .. levels - 1 occurs), offsets[levels] = n.
__global__ __launch_bounds__(kBlock) void derive_offsets_kernel(const int32_t* sortedHeights, int n, int32_t* offsets,
                                                                int levels) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) offsets[levels] = n;
    if (i >= n) return;
    const int32_t h = sortedHeights[i];
    if ((uint32_t)h < (uint32_t)levels && (i == 0 || sortedHeights[i - 1] != h)) offsets[h] = i;
}

__global__ __launch_bounds__(kBlock) void derive_emit_kernel(wide::Derive d) {
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= d.numNodes) return;
    uint32_t o[32];
    int32_t src[4], w = 0;
    if (!wide::step_emit(d, n, o, src, &w)) return;
    uint4* out = reinterpret_cast<uint4*>(d.wideOut + (size_t)w * 32);
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    *reinterpret_cast<int4*>(d.srcOut + (size_t)w * 4) = make_int4(src[0], src[1], src[2], src[3]);
}

int blocks_for(int64_t threads) { return (int)((threads + kBlock - 1) / kBlock); }

size_t aligned(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

hipError_t derive_scratch_bytes(int numNodes, int maxLevels, size_t* bytes, size_t* primTempBytes) {
    size_t sortBytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, sortBytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                   (const int32_t*)nullptr, (int32_t*)nullptr, (unsigned)numNodes, 0, 32);
    if (e != hipSuccess) return e;
    *primTempBytes = std::max<size_t>(16, sortBytes);
    const size_t n = (size_t)numNodes;
    // visited, byDepth, height, size, index, entries, keysOut, ids: 8 of n; kids: 4n
    *bytes = 8 * aligned(n * 4) + aligned(n * 16) + aligned(((size_t)maxLevels + 2) * 4) + 256 + aligned(*primTempBytes);
    return hipSuccess;
}

void derive_carve(wide::Derive& d, DeriveScratch& x, int numNodes, int maxLevels, void* scratch, size_t primTempBytes) {
    char* at = static_cast<char*>(scratch);
    const size_t n = (size_t)numNodes;
    auto take = [&](size_t b) {
        char* p = at;
        at += aligned(b);
        return reinterpret_cast<int32_t*>(p);
    };
    d.numNodes = numNodes;
    d.kids = take(n * 16);
    d.visited = take(n * 4);
    d.byDepth = take(n * 4);
    d.height = take(n * 4);
    d.size = take(n * 4);
    d.index = take(n * 4);
    d.entries = take(n * 4);
    x.keysOut = take(n * 4);
    x.ids = take(n * 4);
    x.depthOffsets = take(((size_t)maxLevels + 2) * 4);
    d.summary = take(256);
    x.primTemp = at;
    x.primTempBytes = primTempBytes;
}

hipError_t launch_derive_init(const wide::Derive& d, const DeriveScratch& x, hipStream_t s) {
    hipLaunchKernelGGL(derive_init_kernel, dim3(blocks_for(std::max(d.numNodes, (int)wide::kSummaryWords))), dim3(kBlock),
                       0, s, d, x.ids);
    return hipGetLastError();
}

hipError_t launch_derive_expand(const wide::Derive& d, int32_t* depthOffsets, int level, int begin, int count,
                                hipStream_t s) {
    if (count <= 0 || begin < 0 || (int64_t)begin + count > d.numNodes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(derive_expand_kernel, dim3(blocks_for(count)), dim3(kBlock), 0, s, d, depthOffsets, level, begin,
                       count);
    return hipGetLastError();
}

hipError_t launch_derive_expand_chain(const wide::Derive& d, int32_t* depthOffsets, int level, int begin, int end,
                                      int maxLevels, hipStream_t s) {
    if (begin < 0 || end < begin || end > d.numNodes || level < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(derive_expand_chain_kernel, dim3(1), dim3(kDeriveChainNodes), 0, s, d, depthOffsets, level, begin,
                       end, maxLevels);
    return hipGetLastError();
}

hipError_t launch_derive_level(DeriveStep step, const wide::Derive& d, int begin, int count, hipStream_t s) {
    if (count <= 0 || begin < 0 || (int64_t)begin + count > d.numNodes) return hipErrorInvalidValue;
    const dim3 grid(blocks_for(count)), block(kBlock);
    switch (step) {
    case kStepHeight: hipLaunchKernelGGL(derive_level_kernel<kStepHeight>, grid, block, 0, s, d, begin, count); break;
    case kStepFlag: hipLaunchKernelGGL(derive_level_kernel<kStepFlag>, grid, block, 0, s, d, begin, count); break;
    case kStepSize: hipLaunchKernelGGL(derive_level_kernel<kStepSize>, grid, block, 0, s, d, begin, count); break;
    case kStepIndex: hipLaunchKernelGGL(derive_level_kernel<kStepIndex>, grid, block, 0, s, d, begin, count); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_derive_chain(DeriveStep step, const wide::Derive& d, const int32_t* depthOffsets, int first,
                               int last, int dir, hipStream_t s) {
    if (first < 0 || last <= first) return hipErrorInvalidValue;
    const dim3 grid(1), block(kDeriveChainNodes);
    switch (step) {
    case kStepHeight:
        hipLaunchKernelGGL(derive_chain_kernel<kStepHeight>, grid, block, 0, s, d, depthOffsets, first, last, dir);
        break;
    case kStepFlag:
        hipLaunchKernelGGL(derive_chain_kernel<kStepFlag>, grid, block, 0, s, d, depthOffsets, first, last, dir);
        break;
    case kStepSize:
        hipLaunchKernelGGL(derive_chain_kernel<kStepSize>, grid, block, 0, s, d, depthOffsets, first, last, dir);
        break;
    case kStepIndex:
        hipLaunchKernelGGL(derive_chain_kernel<kStepIndex>, grid, block, 0, s, d, depthOffsets, first, last, dir);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_derive_sort(const wide::Derive& d, const DeriveScratch& x, int32_t* order, int32_t* offsets,
                              int levels, hipStream_t s) {
    if (levels < 1 || levels > d.numNodes) return hipErrorInvalidValue;
    size_t bytes = x.primTempBytes;
    hipError_t e = rocprim::radix_sort_pairs(x.primTemp, bytes, reinterpret_cast<const uint32_t*>(d.height),
                                             reinterpret_cast<uint32_t*>(x.keysOut), x.ids, order, (unsigned)d.numNodes, 0,
                                             32, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(offsets, 0xff, ((size_t)levels + 1) * 4, s);   // a height that does not occur stays -1
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(derive_offsets_kernel, dim3(blocks_for(d.numNodes)), dim3(kBlock), 0, s, x.keysOut, d.numNodes,
                       offsets, levels);
    return hipGetLastError();
}

hipError_t launch_derive_emit(const wide::Derive& d, hipStream_t s) {
    if (d.numWide <= 0 || !d.wideOut || !d.srcOut) return hipErrorInvalidValue;
    hipLaunchKernelGGL(derive_emit_kernel, dim3(blocks_for(d.numNodes)), dim3(kBlock), 0, s, d);
    return hipGetLastError();
}

}  // namespace mrt
