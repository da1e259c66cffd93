// refit_kernel.hip — gfx950 kernels that refit the bound Compact2 BVH in place for
// moved vertices of a fixed topology (mrt_tracer_refit; the CPU statement is
// csrc/host/refit.cpp, the arithmetic woop_common.hpp's on both sides).
//
// A refit is a short chain of launches on the caller's stream:
//   refit_leaves   one thread per (node, leaf child): the leaf's Woop rows from its
//                  triangles' new vertices, its box into the parent's slot
//   refit_level    one launch per height level >= 1 with more than kRefitTailNodes
//                  nodes: one thread per node, the union of each inner child's two boxes
//   refit_tail     every remaining level in ONE workgroup, a barrier between levels
//                  (level sizes never grow with the height, so the small levels are
//                  the last ones)
//   refit_wide     one thread per child of the derived exact 4-wide array: its six
//                  planes copied from the Compact2 slot the collapse took them from
// A thread reads only bytes written by EARLIER launches, or (refit_tail) by its own
// workgroup before a barrier: no workgroup waits on or reads another's output inside a
// launch. The per-XCD L2s and per-CU L1s make such hand-offs a hazard; a kernel
// boundary costs a few microseconds and is always right.
//
// This file is built WITHOUT -fgpu-flush-denormals-to-zero (Makefile), and division
// is hipcc's default correctly rounded one, so every float here is the IEEE value the
// host computes: the Woop rows come out bit for bit, denormal, infinite and +-0 rows
// included. Only the bits of a NaN that an operation makes differ (x86 0xFFC00000,
// gfx950 0x7FC00000). A NaN vertex coordinate enters no box (woop_common.hpp).
//
// Every index read from memory is range-checked before it is used as one: a leaf
// that runs past the Woop array ends there, a triIndex entry or vertex index out of
// range skips that triangle (its rows stay as they were) and is counted.
#include "refit_kernel.hpp"
#include "woop_common.hpp"

namespace mrt {

namespace {

constexpr int kRefitBlock = 256;

__device__ __forceinline__ void store_box(uint32_t* rec, int side, const woop::Box& b) {
    *reinterpret_cast<float4*>(rec + 4 * side) = make_float4(b.lo[0], b.hi[0], b.lo[1], b.hi[1]);
    *reinterpret_cast<float2*>(rec + 8 + 2 * side) = make_float2(b.lo[2], b.hi[2]);
}

__global__ __launch_bounds__(kRefitBlock) void refit_leaves_kernel(RefitArgs a) {
    const int g = blockIdx.x * kRefitBlock + threadIdx.x;
    if (g >= 2 * a.numNodes) return;
    const int side = g & 1;
    uint32_t* rec = a.nodes + (size_t)(g >> 1) * 16;
    const int32_t ref = (int32_t)rec[12 + side];
    if (ref >= 0) return;   // an inner child: its box and valid flag are the level launches'

    woop::Box box = woop::box_empty();
    bool any = false;
    unsigned skipped = 0;
    // Z rows only, in steps of three from the leaf's first slot: a U or V row may hold -0.0 too.
    for (int64_t s = ~(int64_t)ref; s < a.woopSlots; s += 3) {
        if (a.woop[s * 4] == woop::kTerminatorBits || s + 2 >= a.woopSlots) break;
        const int32_t tri = a.triIndex[s];
        if ((uint64_t)(int64_t)tri >= (uint64_t)a.numTriangles) {
            skipped++;
            continue;
        }
        const int32_t* t = a.triangles + (size_t)tri * 3;
        const int32_t i0 = t[0], i1 = t[1], i2 = t[2];
        const uint64_t nv = (uint64_t)a.numVertices;
        if ((uint64_t)(int64_t)i0 >= nv || (uint64_t)(int64_t)i1 >= nv || (uint64_t)(int64_t)i2 >= nv) {
            skipped++;
            continue;
        }
        const float* p0 = a.vertices + (size_t)i0 * 3;
        const float* p1 = a.vertices + (size_t)i1 * 3;
        const float* p2 = a.vertices + (size_t)i2 * 3;
        const float v0[3] = {p0[0], p0[1], p0[2]}, v1[3] = {p1[0], p1[1], p1[2]}, v2[3] = {p2[0], p2[1], p2[2]};
        float rows[12];
        woop::woop_rows(v0, v1, v2, rows);
        woop::woop_guard(rows);
        float4* w = reinterpret_cast<float4*>(a.woop) + s;
        w[0] = make_float4(rows[0], rows[1], rows[2], rows[3]);
        w[1] = make_float4(rows[4], rows[5], rows[6], rows[7]);
        w[2] = make_float4(rows[8], rows[9], rows[10], rows[11]);
        woop::box_grow(box, v0);
        woop::box_grow(box, v1);
        woop::box_grow(box, v2);
        any = true;
    }
    if (skipped) atomicAdd(a.skipped, (unsigned long long)skipped);
    a.valid[g] = any ? 1 : 0;
    if (any) store_box(rec, side, box);   // an empty leaf keeps its stored box
}

// The boxes of node n's inner children, each the union of that child record's two boxes.
__device__ __forceinline__ void refit_node(const RefitArgs& a, int n) {
    if ((unsigned)n >= (unsigned)a.numNodes) return;
    uint32_t* rec = a.nodes + (size_t)n * 16;
    for (int side = 0; side < 2; side++) {
        const int32_t ref = (int32_t)rec[12 + side];
        if (ref < 0) continue;
        const int child = ref >> 2;
        if ((ref & 3) || child >= a.numNodes) continue;
        const float4* c = reinterpret_cast<const float4*>(a.nodes + (size_t)child * 16);
        const float4 q0 = c[0], q1 = c[1], q2 = c[2];
        const bool v0 = a.valid[2 * child] != 0, v1 = a.valid[2 * child + 1] != 0;
        a.valid[2 * n + side] = (v0 || v1) ? 1 : 0;
        if (!v0 && !v1) continue;   // nothing but empty leaves below: the stored box stays
        const woop::Box b0{{q0.x, q0.z, q2.x}, {q0.y, q0.w, q2.y}};
        const woop::Box b1{{q1.x, q1.z, q2.z}, {q1.y, q1.w, q2.w}};
        store_box(rec, side, v0 && v1 ? woop::box_union(b0, b1) : (v0 ? b0 : b1));
    }
}

__global__ __launch_bounds__(kRefitBlock) void refit_level_kernel(RefitArgs a, const int32_t* order, int begin, int count) {
    const int i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < count) refit_node(a, order[begin + i]);
}

__global__ __launch_bounds__(kRefitTailNodes) void refit_tail_kernel(RefitArgs a, const int32_t* order,
                                                                     const int32_t* offsets, int firstLevel,
                                                                     int numLevels) {
    for (int l = firstLevel; l < numLevels; l++) {
        const int end = offsets[l + 1];
        for (int i = offsets[l] + (int)threadIdx.x; i < end; i += kRefitTailNodes) refit_node(a, order[i]);
        __syncthreads();   // this workgroup's stores of level l before its loads of level l + 1
    }
}

__global__ __launch_bounds__(kRefitBlock) void refit_wide_kernel(RefitArgs a, const int32_t* wideSrc, uint32_t* wide,
                                                                 int numWide) {
    const int g = blockIdx.x * kRefitBlock + threadIdx.x;
    if (g >= 4 * numWide) return;
    const int32_t src = wideSrc[g];
    if (src < 0 || (src >> 1) >= a.numNodes) return;   // an absent child: NaN planes and the sentinel stay
    const int side = src & 1, c = g & 3;
    const uint32_t* rec = a.nodes + (size_t)(src >> 1) * 16;
    const float2 x = *reinterpret_cast<const float2*>(rec + 4 * side);
    const float2 y = *reinterpret_cast<const float2*>(rec + 4 * side + 2);
    const float2 z = *reinterpret_cast<const float2*>(rec + 8 + 2 * side);
    uint32_t* o = wide + (size_t)(g >> 2) * 32 + (c >> 1) * 4 + (c & 1) * 2;   // children 0,1 in float4 0/2/4, 2,3 in 1/3/5
    *reinterpret_cast<float2*>(o) = x;
    *reinterpret_cast<float2*>(o + 8) = y;
    *reinterpret_cast<float2*>(o + 16) = z;
}

int blocks_for(int64_t threads) { return (int)((threads + kRefitBlock - 1) / kRefitBlock); }

}  // namespace

hipError_t launch_refit_leaves(const RefitArgs& a, hipStream_t s) {
    if (a.numNodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_leaves_kernel, dim3(blocks_for(2 * (int64_t)a.numNodes)), dim3(kRefitBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_refit_level(const RefitArgs& a, const int32_t* order, int begin, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_level_kernel, dim3(blocks_for(count)), dim3(kRefitBlock), 0, s, a, order, begin, count);
    return hipGetLastError();
}

hipError_t launch_refit_tail(const RefitArgs& a, const int32_t* order, const int32_t* offsets, int firstLevel,
                             int numLevels, hipStream_t s) {
    if (firstLevel >= numLevels) return hipSuccess;
    hipLaunchKernelGGL(refit_tail_kernel, dim3(1), dim3(kRefitTailNodes), 0, s, a, order, offsets, firstLevel, numLevels);
    return hipGetLastError();
}

hipError_t launch_refit_wide(const RefitArgs& a, const int32_t* wideSrc, uint32_t* wideNodes, int numWide,
                             hipStream_t s) {
    if (numWide <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_wide_kernel, dim3(blocks_for(4 * (int64_t)numWide)), dim3(kRefitBlock), 0, s, a, wideSrc,
                       wideNodes, numWide);
    return hipGetLastError();
}

}  // namespace mrt
