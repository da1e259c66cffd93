// lbvh_kernel.hip — gfx950 kernels that build the topology of a linear BVH (Morton
// order, Karras 2012 hierarchy, leaves of at most maxLeaf triangles) from device
// vertex / triangle arrays straight into Compact2 buffers (mrt_tracer_build; the CPU
// statement is csrc/host/lbvh.cpp, the arithmetic lbvh_common.hpp's on both sides).
//
// A build is a chain of launches on the caller's stream:
//   lbvh_bounds_partial  per block the min / max of its triangles' centroids
//   lbvh_bounds_final    one workgroup: the min / max of the partials
//   lbvh_keys            one thread per triangle: its 63-bit Morton code, its id
//   (rocPRIM)            stable radix sort of (code, id)
//   lbvh_hierarchy       one thread per internal node: range and split by binary
//                        search on delta over the sorted codes
//   lbvh_flags           one thread per internal node: kept (more than maxLeaf
//                        triangles), and a leaf-start flag per child range of a kept
//                        node that holds at most maxLeaf
//   (rocPRIM)            exclusive sums of both flag arrays: record numbers, leaf ranks
//   lbvh_emit_records    one thread per internal node: a kept node's record (child
//                        refs, zeroed boxes)
//   lbvh_emit_slots      one thread per sorted position: three zeroed Woop slots, the
//                        triangle id at the Z row's slot, the leaf's terminator
// Boxes and Woop rows are then the refit launches' (refit_kernel.hip). A thread reads
// only what EARLIER launches wrote (lbvh_bounds_final: what one workgroup read itself);
// every dependency is a kernel boundary (the per-XCD L2 reason of refit_kernel.hip).
//
// Built WITHOUT -fgpu-flush-denormals-to-zero and with correctly rounded division
// (Makefile), so the keys are the host's bit for bit, for denormal, infinite and NaN
// coordinates too (a NaN centroid enters no bounds and quantizes to 0). A triangle with a vertex index
// outside [0, numVertices) gets code 0 and its vertices are never read. Every index
// computed from scratch is range-checked before it addresses an output.
#include "lbvh_kernel.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "lbvh_common.hpp"

namespace mrt {

namespace {

constexpr int kBlock = 256;
constexpr int kBoundsBlocks = 1024;   // at most this many partials

__device__ __forceinline__ bool load_centroid(const LbvhBuild& b, int i, float c[3]) {
    const int32_t* t = b.triangles + (size_t)i * 3;
    const int32_t idx[3] = {t[0], t[1], t[2]};
    if (!lbvh::tri_in_range(idx, b.numVertices)) return false;
    const float* p0 = b.vertices + (size_t)idx[0] * 3;
    const float* p1 = b.vertices + (size_t)idx[1] * 3;
    const float* p2 = b.vertices + (size_t)idx[2] * 3;
    const float v0[3] = {p0[0], p0[1], p0[2]}, v1[3] = {p1[0], p1[1], p1[2]}, v2[3] = {p2[0], p2[1], p2[2]};
    lbvh::tri_centroid(v0, v1, v2, c);
    return true;
}

// The workgroup's merged bounds, valid in thread 0.
__device__ __forceinline__ lbvh::Bounds block_bounds(lbvh::Bounds mine) {
    __shared__ lbvh::Bounds sh[kBlock];
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lbvh::bounds_merge(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ void store_bounds(float* out, const lbvh::Bounds& b) {
    for (int k = 0; k < 3; k++) {
        out[k] = b.lo[k];
        out[3 + k] = b.hi[k];
    }
}

__global__ __launch_bounds__(kBlock) void lbvh_bounds_partial_kernel(LbvhBuild b) {
    lbvh::Bounds mine = lbvh::bounds_empty();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < b.numTriangles; i += (int64_t)gridDim.x * kBlock) {
        float c[3];
        if (load_centroid(b, (int)i, c)) lbvh::bounds_grow(mine, c);
    }
    const lbvh::Bounds all = block_bounds(mine);
    if (threadIdx.x == 0) store_bounds(b.partial + (size_t)blockIdx.x * 6, all);
}

__global__ __launch_bounds__(kBlock) void lbvh_bounds_final_kernel(LbvhBuild b, int numPartials) {
    lbvh::Bounds mine = lbvh::bounds_empty();
    for (int i = threadIdx.x; i < numPartials; i += kBlock) {
        const float* p = b.partial + (size_t)i * 6;
        const lbvh::Bounds o{{p[0], p[1], p[2]}, {p[3], p[4], p[5]}};
        lbvh::bounds_merge(mine, o);
    }
    const lbvh::Bounds all = block_bounds(mine);
    if (threadIdx.x == 0) store_bounds(b.bounds, all);
}

__global__ __launch_bounds__(kBlock) void lbvh_keys_kernel(LbvhBuild b) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= b.numTriangles) return;
    const lbvh::Bounds all{{b.bounds[0], b.bounds[1], b.bounds[2]}, {b.bounds[3], b.bounds[4], b.bounds[5]}};
    float c[3];
    b.codes[i] = load_centroid(b, i, c) ? lbvh::tri_code(c, all) : 0;
    b.ids[i] = i;
}

__global__ __launch_bounds__(kBlock) void lbvh_hierarchy_kernel(LbvhBuild b) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= b.numTriangles - 1) return;
    const lbvh::Node n = lbvh::karras_node(b.codesSorted, b.numTriangles, k);
    b.first[k] = n.first;
    b.last[k] = n.last;
    b.split[k] = n.split;
}

// A node's range and split as the hierarchy launch stored them, checked: first <= split < last < n.
__device__ __forceinline__ bool load_node(const LbvhBuild& b, int k, lbvh::Node* n) {
    n->first = b.first[k];
    n->last = b.last[k];
    n->split = b.split[k];
    return n->first >= 0 && n->first <= n->split && n->split < n->last && n->last < b.numTriangles;
}

// kept and leafStart are zeroed before this launch; leaf starts are distinct positions.
__global__ __launch_bounds__(kBlock) void lbvh_flags_kernel(LbvhBuild b) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= b.numTriangles - 1) return;
    lbvh::Node n;
    if (!load_node(b, k, &n) || n.last - n.first + 1 <= b.maxLeaf) return;
    b.kept[k] = 1;
    if (n.split - n.first + 1 <= b.maxLeaf) b.leafStart[n.first] = 1;
    if (n.last - n.split <= b.maxLeaf) b.leafStart[n.split + 1] = 1;
}

__global__ __launch_bounds__(kBlock) void lbvh_emit_records_kernel(LbvhBuild b) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const int n = b.numTriangles;
    if (k >= n - 1 || !b.kept[k]) return;
    lbvh::Node nd;
    const int rec = b.keptRank[k];
    if (!load_node(b, k, &nd) || (unsigned)rec >= (unsigned)(n - 1)) return;
    // child i covers [from, to]; more than one position: Karras node `node`
    const int from[2] = {nd.first, nd.split + 1}, to[2] = {nd.split, nd.last}, node[2] = {nd.split, nd.split + 1};
    int32_t ref[2];
    for (int i = 0; i < 2; i++) {
        if (to[i] - from[i] + 1 > b.maxLeaf) {
            const int child = b.keptRank[node[i]];
            ref[i] = (unsigned)child < (unsigned)(n - 1) ? child * 4 : 0;
        } else {
            const int rank = b.leafRank[from[i]];
            ref[i] = ~lbvh::leaf_slot(from[i], (unsigned)rank <= (unsigned)from[i] ? rank : 0);
        }
    }
    uint4* out = reinterpret_cast<uint4*>(b.nodes + (size_t)rec * 16);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    out[0] = zero;
    out[1] = zero;
    out[2] = zero;
    out[3] = make_uint4((uint32_t)ref[0], (uint32_t)ref[1], 0, 0);
}

// single: all triangles in the one leaf of rank 0 (at most maxLeaf triangles).
template <bool kSingle>
__global__ __launch_bounds__(kBlock) void lbvh_emit_slots_kernel(LbvhBuild b) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int n = b.numTriangles;
    if (p >= n) return;
    const int rank = kSingle ? 0 : b.leafRank[p] + b.leafStart[p] - 1;   // of the leaf p lies in
    if ((unsigned)rank > (unsigned)p) return;                            // slots stay inside 4n
    const bool ends = p == n - 1 || (!kSingle && b.leafStart[p + 1] != 0);
    const int slot = lbvh::leaf_slot(p, rank);
    uint4* w = reinterpret_cast<uint4*>(b.woop) + slot;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    w[0] = zero;   // the rows are the refit launch's; an out-of-range triangle keeps these
    w[1] = zero;
    w[2] = zero;
    const int32_t id = b.idsSorted[p];
    b.triIndex[slot] = (unsigned)id < (unsigned)n ? id : 0;
    b.triIndex[slot + 1] = 0;
    b.triIndex[slot + 2] = 0;
    if (ends) {
        const uint32_t t = woop::kTerminatorBits;
        w[3] = make_uint4(t, t, t, t);
        b.triIndex[slot + 3] = 0;
    }
    if (kSingle && p == 0) {
        // the record, and the empty leaf: a lone terminator after child 0's
        const uint32_t t = woop::kTerminatorBits;
        const int empty = 3 * n + 1;
        reinterpret_cast<uint4*>(b.woop)[empty] = make_uint4(t, t, t, t);
        b.triIndex[empty] = 0;
        uint4* out = reinterpret_cast<uint4*>(b.nodes);
        out[0] = zero;
        out[1] = zero;
        out[2] = zero;
        out[3] = make_uint4((uint32_t)~0, (uint32_t)~empty, 0, 0);
    }
}

__global__ void lbvh_empty_leaf_box_kernel(uint32_t* nodes) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < 3; k++) {
        nodes[woop::box_word(1, k)] = nodes[woop::box_word(0, k)];
        nodes[woop::box_word(1, k) + 1] = nodes[woop::box_word(0, k) + 1];
    }
}

int blocks_for(int64_t threads) { return (int)((threads + kBlock - 1) / kBlock); }
int bounds_blocks(int n) { return std::min(kBoundsBlocks, blocks_for(n)); }

size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// The byte offset of every scratch array, in LbvhBuild's order; returns the total.
struct Layout {
    size_t partial, bounds, codes, codesSorted, ids, idsSorted, first, last, split, kept, leafStart, keptRank, leafRank,
        primTemp, total;
};
Layout layout(int n, size_t primTempBytes) {
    Layout l{};
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += aligned(bytes);
        return here;
    };
    const size_t N = (size_t)n;
    l.codes = take(N * 8);
    l.codesSorted = take(N * 8);
    l.partial = take((size_t)kBoundsBlocks * 6 * 4);
    l.bounds = take(6 * 4);
    l.ids = take(N * 4);
    l.idsSorted = take(N * 4);
    l.first = take(N * 4);
    l.last = take(N * 4);
    l.split = take(N * 4);
    l.kept = take(N * 4);   // kept and leafStart are zeroed by one memset: keep them adjacent
    l.leafStart = take((N + 1) * 4);
    l.keptRank = take(N * 4);
    l.leafRank = take((N + 1) * 4);
    l.primTemp = take(primTempBytes);
    l.total = at;
    return l;
}

}  // namespace

hipError_t lbvh_scratch_bytes(int numTriangles, size_t* bytes, size_t* primTempBytes) {
    const unsigned n = (unsigned)numTriangles;
    size_t sortBytes = 0, scanBytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sortBytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                             (const int32_t*)nullptr, (int32_t*)nullptr, n, 0, 63);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, scanBytes, (const int32_t*)nullptr, (int32_t*)nullptr, 0, n + 1,
                                rocprim::plus<int32_t>());
    if (e != hipSuccess) return e;
    *primTempBytes = std::max<size_t>(16, std::max(sortBytes, scanBytes));
    *bytes = layout(numTriangles, *primTempBytes).total;
    return hipSuccess;
}

void lbvh_carve(LbvhBuild& b, void* scratch, size_t primTempBytes) {
    const Layout l = layout(b.numTriangles, primTempBytes);
    char* base = static_cast<char*>(scratch);
    b.partial = reinterpret_cast<float*>(base + l.partial);
    b.bounds = reinterpret_cast<float*>(base + l.bounds);
    b.codes = reinterpret_cast<uint64_t*>(base + l.codes);
    b.codesSorted = reinterpret_cast<uint64_t*>(base + l.codesSorted);
    b.ids = reinterpret_cast<int32_t*>(base + l.ids);
    b.idsSorted = reinterpret_cast<int32_t*>(base + l.idsSorted);
    b.first = reinterpret_cast<int32_t*>(base + l.first);
    b.last = reinterpret_cast<int32_t*>(base + l.last);
    b.split = reinterpret_cast<int32_t*>(base + l.split);
    b.kept = reinterpret_cast<int32_t*>(base + l.kept);
    b.leafStart = reinterpret_cast<int32_t*>(base + l.leafStart);
    b.keptRank = reinterpret_cast<int32_t*>(base + l.keptRank);
    b.leafRank = reinterpret_cast<int32_t*>(base + l.leafRank);
    b.primTemp = base + l.primTemp;
    b.primTempBytes = primTempBytes;
}

hipError_t launch_lbvh_sort(const LbvhBuild& b, hipStream_t s) {
    const int n = b.numTriangles;
    const int partials = bounds_blocks(n);
    hipLaunchKernelGGL(lbvh_bounds_partial_kernel, dim3(partials), dim3(kBlock), 0, s, b);
    hipLaunchKernelGGL(lbvh_bounds_final_kernel, dim3(1), dim3(kBlock), 0, s, b, partials);
    hipLaunchKernelGGL(lbvh_keys_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = b.primTempBytes;
    return rocprim::radix_sort_pairs(b.primTemp, bytes, b.codes, b.codesSorted, b.ids, b.idsSorted, (unsigned)n, 0, 63, s);
}

hipError_t launch_lbvh_emit(const LbvhBuild& b, hipStream_t s) {
    const int n = b.numTriangles;
    if (n < 2) return hipErrorInvalidValue;
    const int nodeBlocks = blocks_for(n - 1);
    hipLaunchKernelGGL(lbvh_hierarchy_kernel, dim3(nodeBlocks), dim3(kBlock), 0, s, b);
    // kept (n) and leafStart (n + 1) with the padding between them
    hipError_t e = hipMemsetAsync(b.kept, 0, (size_t)((char*)(b.leafStart + n + 1) - (char*)b.kept), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lbvh_flags_kernel, dim3(nodeBlocks), dim3(kBlock), 0, s, b);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = b.primTempBytes;
    e = rocprim::exclusive_scan(b.primTemp, bytes, b.kept, b.keptRank, 0, (unsigned)n, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    bytes = b.primTempBytes;
    e = rocprim::exclusive_scan(b.primTemp, bytes, b.leafStart, b.leafRank, 0, (unsigned)n + 1, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lbvh_emit_records_kernel, dim3(nodeBlocks), dim3(kBlock), 0, s, b);
    hipLaunchKernelGGL(lbvh_emit_slots_kernel<false>, dim3(blocks_for(n)), dim3(kBlock), 0, s, b);
    return hipGetLastError();
}

hipError_t launch_lbvh_emit_single(const LbvhBuild& b, hipStream_t s) {
    hipLaunchKernelGGL(lbvh_emit_slots_kernel<true>, dim3(blocks_for(b.numTriangles)), dim3(kBlock), 0, s, b);
    return hipGetLastError();
}

hipError_t launch_lbvh_empty_leaf_box(uint32_t* nodes, hipStream_t s) {
    hipLaunchKernelGGL(lbvh_empty_leaf_box_kernel, dim3(1), dim3(64), 0, s, nodes);
    return hipGetLastError();
}

}  // namespace mrt
