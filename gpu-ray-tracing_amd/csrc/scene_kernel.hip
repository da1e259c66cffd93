// scene_kernel.hip — gfx950 kernels for what a moving scene needs beside its tree:
//   scene_attributes   one lane per triangle: the face normal and the shaded / material colours
//                      from device vertices (mrt_scene_attributes; the CPU statement is
//                      csrc/host/scene_attr.cpp, the arithmetic scene_common.hpp's on both sides)
//   tree_cost_partial  one lane per child slot of the bound Compact2 records: its area term, a
//                      leaf's triangle count; a DPP reduction per wave, the waves of a workgroup
//                      added in wave order, one partial per workgroup
//   tree_cost_final    one wave: lane j adds a contiguous run of partials in index order, the
//                      lanes are added by the same DPP reduction, record 0's root term joins
// No floating-point atomic anywhere: the order of every addition is fixed by the record count
// alone, so two runs on the same tree give the same bits.
//
// This file is built WITHOUT -fgpu-flush-denormals-to-zero (Makefile), with -ffp-contract=off and
// hipcc's default correctly rounded division and square root: every float is the IEEE value the
// host computes, denormals included. Only the bits of a NaN that an operation makes differ.
//
// Every index read from memory is range-checked before it is used as one: a triangle with a
// vertex index out of range reads no vertex, a leaf's walk ends with the Woop array.
#include "scene_kernel.hpp"
#include "scene_common.hpp"

namespace mrt {

namespace {

constexpr int kWave = 64;
static_assert(kSceneBlock % kWave == 0 && kCostFinalLanes == kWave, "whole waves");

__global__ __launch_bounds__(kSceneBlock) void scene_attributes_kernel(SceneAttrArgs a) {
    __shared__ float stage[3 * kSceneBlock];
    const int tid = threadIdx.x;
    const int base = blockIdx.x * kSceneBlock;
    const int i = base + tid;
    const bool live = i < a.numTriangles;
    float n[3] = {0.0f, 0.0f, 0.0f};
    bool skip = false;
    if (live) {
        const int32_t* t = a.triangles + (size_t)i * 3;
        const int32_t i0 = t[0], i1 = t[1], i2 = t[2];
        const uint64_t nv = (uint64_t)a.numVertices;
        skip = (uint64_t)(int64_t)i0 >= nv || (uint64_t)(int64_t)i1 >= nv || (uint64_t)(int64_t)i2 >= nv;
        if (!skip) {
            const float* p0 = a.vertices + (size_t)i0 * 3;
            const float* p1 = a.vertices + (size_t)i1 * 3;
            const float* p2 = a.vertices + (size_t)i2 * 3;
            const float v0[3] = {p0[0], p0[1], p0[2]}, v1[3] = {p1[0], p1[1], p1[2]}, v2[3] = {p2[0], p2[1], p2[2]};
            scene::tri_normal(v0, v1, v2, n);
        }
    }
    // One integer atomic per wave that skipped something. No lane has left: lane 0 is there.
    const unsigned long long skippers = __ballot(skip);
    if (a.skipped && skippers && (tid & (kWave - 1)) == 0) atomicAdd(a.skipped, (unsigned long long)__popcll(skippers));

    if (live && (a.triShadedColor || a.triMaterialColor)) {
        float diffuse[4];
        if (a.triDiffuse) {
            const float* d = a.triDiffuse + (size_t)i * 4;
            diffuse[0] = d[0], diffuse[1] = d[1], diffuse[2] = d[2], diffuse[3] = d[3];
        } else {
            scene::default_diffuse(diffuse);
        }
        if (a.triMaterialColor) a.triMaterialColor[i] = scene::to_abgr(diffuse);
        if (a.triShadedColor) {
            float light[3];
            scene::light_dir(light);
            a.triShadedColor[i] = scene::shade(n, light, diffuse);
        }
    }
    if (a.triNormals) {   // uniform: through LDS, so that every store instruction writes consecutive words
        stage[3 * tid] = n[0];
        stage[3 * tid + 1] = n[1];
        stage[3 * tid + 2] = n[2];
        __syncthreads();
        const int left = a.numTriangles - base;
        const int words = 3 * (left < kSceneBlock ? left : kSceneBlock);
        float* out = a.triNormals + (size_t)base * 3;
        for (int k = tid; k < words; k += kSceneBlock) out[k] = stage[k];
    }
}

// v of the lane a DPP control names, 0 where it names none or the row is masked off.
template <int Ctrl, int RowMask>
__device__ __forceinline__ int dpp_or_zero(int v) {
    return __builtin_amdgcn_update_dpp(0, v, Ctrl, RowMask, 0xf, false);
}
template <int Ctrl, int RowMask>
__device__ __forceinline__ double dpp_add(double x) {
    const int hi = dpp_or_zero<Ctrl, RowMask>(__double2hiint(x)), lo = dpp_or_zero<Ctrl, RowMask>(__double2loint(x));
    return x + __hiloint2double(hi, lo);
}
template <int Ctrl, int RowMask>
__device__ __forceinline__ long long dpp_add(long long x) {
    const int hi = dpp_or_zero<Ctrl, RowMask>((int)(x >> 32)), lo = dpp_or_zero<Ctrl, RowMask>((int)x);
    return x + (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// The sum over a full wave, in lane 63: an inclusive scan inside each row of 16 lanes (row_shr 1,
// 2, 4, 8), then row 0's total into row 1 and row 2's into row 3 (row_bcast:15), then lane 31's
// into rows 2 and 3 (row_bcast:31). All 64 lanes must be active.
template <class T>
__device__ __forceinline__ T wave_sum_in_last_lane(T x) {
    x = dpp_add<0x111, 0xf>(x);
    x = dpp_add<0x112, 0xf>(x);
    x = dpp_add<0x114, 0xf>(x);
    x = dpp_add<0x118, 0xf>(x);
    x = dpp_add<0x142, 0xa>(x);
    x = dpp_add<0x143, 0xc>(x);
    return x;
}

__device__ __forceinline__ CostPartial wave_sum_in_last_lane(const CostPartial& p) {
    CostPartial r;
    r.inner = wave_sum_in_last_lane(p.inner);
    r.leaf = wave_sum_in_last_lane(p.leaf);
    r.leafTri = wave_sum_in_last_lane(p.leafTri);
    r.leaves = wave_sum_in_last_lane(p.leaves);
    r.triangles = wave_sum_in_last_lane(p.triangles);
    r.skipped = wave_sum_in_last_lane(p.skipped);
    return r;
}

__device__ __forceinline__ void add_to(CostPartial& s, const CostPartial& p) {
    s.inner += p.inner;
    s.leaf += p.leaf;
    s.leafTri += p.leafTri;
    s.leaves += p.leaves;
    s.triangles += p.triangles;
    s.skipped += p.skipped;
}

__device__ __forceinline__ woop::Box slot_box(const uint32_t* rec, int side) {
    woop::Box b;
    for (int k = 0; k < 3; k++) {
        const int w = woop::box_word(side, k);
        b.lo[k] = __uint_as_float(rec[w]);
        b.hi[k] = __uint_as_float(rec[w + 1]);
    }
    return b;
}

__global__ __launch_bounds__(kSceneBlock) void tree_cost_partial_kernel(TreeCostArgs a) {
    __shared__ CostPartial waves[kSceneBlock / kWave];
    const int tid = threadIdx.x;
    const int g = blockIdx.x * kSceneBlock + tid;
    CostPartial mine{0.0, 0.0, 0.0, 0, 0, 0};
    if (g < 2 * a.numNodes) {
        const int side = g & 1;
        const uint32_t* rec = a.nodes + (size_t)(g >> 1) * 16;
        const int32_t ref = (int32_t)rec[12 + side];
        double area;
        const bool ok = scene::tree_cost_term(slot_box(rec, side), &area);
        if (!ok) mine.skipped = 1;
        if (ref >= 0) {
            if (ok) mine.inner = area;
        } else {
            const uint32_t* woop = a.woop;
            const int64_t count = scene::leaf_triangles(ref, a.woopSlots, [woop](int64_t s) { return woop[s * 4]; });
            mine.leaves = 1;
            mine.triangles = count;
            if (ok) {
                mine.leaf = area;
                mine.leafTri = area * (double)count;
            }
        }
    }
    const CostPartial w = wave_sum_in_last_lane(mine);
    if ((tid & (kWave - 1)) == kWave - 1) waves[tid / kWave] = w;
    __syncthreads();
    if (tid == 0) {
        CostPartial s = waves[0];
        for (int k = 1; k < kSceneBlock / kWave; k++) add_to(s, waves[k]);
        a.partials[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kCostFinalLanes) void tree_cost_final_kernel(TreeCostArgs a, int numPartials) {
    const int lane = threadIdx.x;
    const int run = (numPartials + kCostFinalLanes - 1) / kCostFinalLanes;
    const int begin = lane * run < numPartials ? lane * run : numPartials;
    const int end = begin + run < numPartials ? begin + run : numPartials;
    CostPartial mine{0.0, 0.0, 0.0, 0, 0, 0};
    for (int k = begin; k < end; k++) add_to(mine, a.partials[k]);
    const CostPartial s = wave_sum_in_last_lane(mine);
    if (lane != kCostFinalLanes - 1) return;
    // The root: the union of record 0's two boxes, as a refit would write it into a parent's slot.
    double root;
    const bool ok = scene::tree_cost_term(woop::box_union(slot_box(a.nodes, 0), slot_box(a.nodes, 1)), &root);
    mrt_tree_cost c;
    c.root_area = ok ? root : 0.0;
    c.inner_area = ok ? s.inner + root : s.inner;
    c.leaf_area = s.leaf;
    c.leaf_tri_area = s.leafTri;
    c.records = a.numNodes;
    c.leaves = s.leaves;
    c.triangles = s.triangles;
    c.skipped = s.skipped + (ok ? 0 : 1);
    *a.out = c;
}

}  // namespace

hipError_t launch_scene_attributes(const SceneAttrArgs& a, hipStream_t s) {
    if (a.numTriangles <= 0) return hipSuccess;
    const int blocks = (a.numTriangles + kSceneBlock - 1) / kSceneBlock;
    hipLaunchKernelGGL(scene_attributes_kernel, dim3(blocks), dim3(kSceneBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tree_cost(const TreeCostArgs& a, hipStream_t s) {
    if (a.numNodes <= 0) return hipErrorInvalidValue;
    const int partials = cost_partials(a.numNodes);
    hipLaunchKernelGGL(tree_cost_partial_kernel, dim3(partials), dim3(kSceneBlock), 0, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(tree_cost_final_kernel, dim3(1), dim3(kCostFinalLanes), 0, s, a, partials);
    return hipGetLastError();
}

}  // namespace mrt
