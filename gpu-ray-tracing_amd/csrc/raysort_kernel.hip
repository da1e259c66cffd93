// raysort_kernel.hip — gfx950 kernels that sort a ray batch by the reference's Morton key
// (mrt_ray_sort; the CPU statement is csrc/host/raysort.cpp, the arithmetic raysort_common.hpp's
// on both sides; the reference's is RayBuffer::mortonSort with findAABBKernel, genMortonKeysKernel
// and reorderRaysKernel, RayBufferKernels.cu:74-200, and a CPU quicksort between two copies).
//
// A sort is a chain of launches on the caller's stream:
//   raysort_box_partial  per block the min / max of its rays' origins (and end points)
//   raysort_box_final    one workgroup: the min / max of the partials (no float atomics)
//   raysort_keys         one thread per ray: its six key words, in input order
//   per pass of the LSD sort (3, 2 or 1 by drop_levels):
//     raysort_gather     one thread per position: the pass's 64-bit word of the key of the ray
//                        the permutation has there so far (the first pass: the identity)
//     (rocPRIM)          stable radix sort of (word, slot) over the bits that can be set
//   raysort_reorder      two threads per output ray: one 16-byte half each, and the id maps
// A thread reads only what EARLIER launches wrote (raysort_box_final: what one workgroup read
// itself); every dependency is a kernel boundary (the per-XCD L2 reason of refit_kernel.hip).
//
// Built WITHOUT -fgpu-flush-denormals-to-zero and with correctly rounded division and square root
// (Makefile), so the keys are the host's bit for bit, for denormal, infinite and NaN rays too.
// Every index read back from scratch is range-checked before it addresses anything.
#include "raysort_kernel.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace mrt {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ void load_ray(const uint4* rays, int64_t i, float ray[8]) {
    const uint4 a = rays[2 * i], b = rays[2 * i + 1];
    ray[0] = __uint_as_float(a.x); ray[1] = __uint_as_float(a.y); ray[2] = __uint_as_float(a.z); ray[3] = __uint_as_float(a.w);
    ray[4] = __uint_as_float(b.x); ray[5] = __uint_as_float(b.y); ray[6] = __uint_as_float(b.z); ray[7] = __uint_as_float(b.w);
}

// The workgroup's merged box, valid in thread 0.
__device__ __forceinline__ raysort::Box block_box(raysort::Box mine) {
    __shared__ raysort::Box sh[kBlock];
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) raysort::box_merge(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ void store_box(float* out, const raysort::Box& b) {
    for (int k = 0; k < 3; k++) {
        out[k] = b.lo[k];
        out[3 + k] = b.hi[k];
    }
}

__global__ __launch_bounds__(kBlock) void raysort_box_partial_kernel(const uint4* rays, int n, int boxMode, float* partial) {
    raysort::Box mine = raysort::box_empty();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        float ray[8];
        load_ray(rays, i, ray);
        raysort::box_grow_ray(mine, ray, boxMode);
    }
    const raysort::Box all = block_box(mine);
    if (threadIdx.x == 0) store_box(partial + (size_t)blockIdx.x * 6, all);
}

__global__ __launch_bounds__(kBlock) void raysort_box_final_kernel(const float* partial, int numPartials, float* box) {
    raysort::Box mine = raysort::box_empty();
    for (int i = threadIdx.x; i < numPartials; i += kBlock) {
        const float* p = partial + (size_t)i * 6;
        const raysort::Box o{{p[0], p[1], p[2]}, {p[3], p[4], p[5]}};
        raysort::box_merge(mine, o);
    }
    const raysort::Box all = block_box(mine);
    if (threadIdx.x == 0) store_box(box, all);
}

__global__ __launch_bounds__(kBlock) void raysort_keys_kernel(const uint4* rays, int n, const float* boxDev,
                                                              raysort::Box boxArg, uint32_t* out, int stride) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    raysort::Box box = boxArg;
    if (boxDev) box = raysort::Box{{boxDev[0], boxDev[1], boxDev[2]}, {boxDev[3], boxDev[4], boxDev[5]}};
    float ray[8];
    load_ray(rays, i, ray);
    uint32_t hash[raysort::kKeyWords];
    raysort::ray_key(ray, box, hash);
    uint32_t* o = out + (size_t)i * stride;
    if (stride == raysort::kKeyWords + 1) *o++ = (uint32_t)i;   // MortonKey::oldSlot
    for (int k = 0; k < raysort::kKeyWords; k++) o[k] = hash[k];
}

// perm NULL: the identity, which is written to permOut for the pass's sort to carry.
__global__ __launch_bounds__(kBlock) void raysort_gather_kernel(const uint32_t* keys, const int32_t* perm, int n,
                                                                int dropLevels, int pass, uint64_t* word, int32_t* permOut) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const int32_t p = perm ? perm[j] : (int32_t)j;
    uint64_t v = 0;
    if ((uint32_t)p < (uint32_t)n) {
        const uint32_t* k = keys + (size_t)p * raysort::kKeyWords;
        const uint32_t hash[raysort::kKeyWords] = {k[0], k[1], k[2], k[3], k[4], k[5]};
        v = raysort::shifted_word(hash, dropLevels, pass);
    }
    word[j] = v;
    if (permOut) permOut[j] = p;
}

// Thread t moves half t & 1 (16 bytes) of output ray t >> 1: a ray is read as two 16-byte loads
// by two neighbouring lanes, and a wave's stores cover 1024 contiguous bytes.
__global__ __launch_bounds__(kBlock) void raysort_reorder_kernel(const uint4* inRays, const int32_t* inSlotToId, int n,
                                                                 const int32_t* perm, int permStride, uint4* outRays,
                                                                 int32_t* outIdToSlot, int32_t* outSlotToId) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t j = t >> 1;
    if (j >= n) return;
    const int half = (int)(t & 1);
    const int32_t p = perm[(size_t)j * permStride];
    if ((uint32_t)p >= (uint32_t)n) return;   // no ray, no id: the slot is left as it was
    outRays[2 * j + half] = inRays[2 * (int64_t)p + half];
    if (half) return;
    const int32_t id = inSlotToId ? inSlotToId[p] : p;
    if (outSlotToId) outSlotToId[j] = id;
    if (outIdToSlot && (uint32_t)id < (uint32_t)n) outIdToSlot[id] = (int32_t)j;
}

int blocks_for(int64_t threads) { return (int)((threads + kBlock - 1) / kBlock); }
int box_blocks(int n) { return std::min(kRaySortBoxBlocks, blocks_for(n)); }

size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// The byte offset of every scratch array; returns the total.
struct Layout {
    size_t word, wordSorted, keys, partial, box, perm, permSorted, primTemp, total;
};
Layout layout(int n, bool ownKeys, bool ownBox, size_t primTempBytes) {
    Layout l{};
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += aligned(bytes);
        return here;
    };
    const size_t N = (size_t)n;
    l.word = take(N * 8);
    l.wordSorted = take(N * 8);
    l.keys = take(ownKeys ? N * raysort::kKeyWords * 4 : 0);
    l.partial = take((size_t)kRaySortBoxBlocks * 6 * 4);
    l.box = take(ownBox ? 6 * 4 : 0);
    l.perm = take(N * 4);
    l.permSorted = take(N * 4);
    l.primTemp = take(primTempBytes);
    l.total = at;
    return l;
}

hipError_t sort_pass(void* temp, size_t& bytes, const uint64_t* in, uint64_t* out, const int32_t* vin, int32_t* vout,
                     int n, int bits, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, bytes, in, out, vin, vout, (unsigned)n, 0u, (unsigned)bits, s);
}

}  // namespace

hipError_t raysort_scratch_bytes(int numRays, int dropLevels, bool ownKeys, bool ownBox, size_t* bytes,
                                 size_t* primTempBytes) {
    size_t most = 16;
    for (int pass = 0; pass < raysort::sort_passes(dropLevels); pass++) {
        size_t b = 0;
        const hipError_t e =
            sort_pass(nullptr, b, nullptr, nullptr, nullptr, nullptr, numRays, raysort::pass_bits(dropLevels, pass), nullptr);
        if (e != hipSuccess) return e;
        most = std::max(most, b);
    }
    *primTempBytes = most;
    *bytes = layout(numRays, ownKeys, ownBox, most).total;
    return hipSuccess;
}

void raysort_carve(RaySort& s, void* scratch, size_t primTempBytes) {
    const Layout l = layout(s.numRays, s.keys == nullptr, s.box == nullptr, primTempBytes);
    char* base = static_cast<char*>(scratch);
    s.word = reinterpret_cast<uint64_t*>(base + l.word);
    s.wordSorted = reinterpret_cast<uint64_t*>(base + l.wordSorted);
    if (!s.keys) s.keys = reinterpret_cast<uint32_t*>(base + l.keys);
    s.partial = reinterpret_cast<float*>(base + l.partial);
    if (!s.box) s.box = reinterpret_cast<float*>(base + l.box);
    s.perm = reinterpret_cast<int32_t*>(base + l.perm);
    s.permSorted = reinterpret_cast<int32_t*>(base + l.permSorted);
    s.primTemp = base + l.primTemp;
    s.primTempBytes = primTempBytes;
}

hipError_t launch_raysort_box(const uint4* rays, int numRays, int boxMode, float* partial, float* box, hipStream_t stream) {
    const int partials = box_blocks(numRays);
    hipLaunchKernelGGL(raysort_box_partial_kernel, dim3(partials), dim3(kBlock), 0, stream, rays, numRays, boxMode, partial);
    hipLaunchKernelGGL(raysort_box_final_kernel, dim3(1), dim3(kBlock), 0, stream, partial, partials, box);
    return hipGetLastError();
}

hipError_t launch_raysort_keys(const uint4* rays, int numRays, const float* boxDev, const raysort::Box& boxHost,
                               uint32_t* out, int stride, hipStream_t stream) {
    if (stride != raysort::kKeyWords && stride != raysort::kKeyWords + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(raysort_keys_kernel, dim3(blocks_for(numRays)), dim3(kBlock), 0, stream, rays, numRays, boxDev,
                       boxHost, out, stride);
    return hipGetLastError();
}

hipError_t launch_raysort_reorder(const uint4* inRays, const int32_t* inSlotToId, int numRays, const int32_t* perm,
                                  int permStride, uint4* outRays, int32_t* outIdToSlot, int32_t* outSlotToId,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(raysort_reorder_kernel, dim3(blocks_for(2 * (int64_t)numRays)), dim3(kBlock), 0, stream, inRays,
                       inSlotToId, numRays, perm, permStride, outRays, outIdToSlot, outSlotToId);
    return hipGetLastError();
}

hipError_t launch_raysort(const RaySort& s, hipStream_t stream) {
    const int n = s.numRays;
    hipError_t e = launch_raysort_box(s.inRays, n, s.boxMode, s.partial, s.box, stream);
    if (e != hipSuccess) return e;
    e = launch_raysort_keys(s.inRays, n, s.box, raysort::box_empty(), s.keys, raysort::kKeyWords, stream);
    if (e != hipSuccess) return e;
    const int32_t* have = nullptr;   // the permutation so far: none yet (the identity)
    int32_t* in = s.perm;
    int32_t* out = s.permSorted;
    for (int pass = 0; pass < raysort::sort_passes(s.dropLevels); pass++) {
        // the first pass's identity is written to `in`; a later pass's values are `have` itself
        hipLaunchKernelGGL(raysort_gather_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, s.keys, have, n,
                           s.dropLevels, pass, s.word, have ? nullptr : in);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t bytes = s.primTempBytes;
        e = sort_pass(s.primTemp, bytes, s.word, s.wordSorted, have ? have : in, out, n,
                      raysort::pass_bits(s.dropLevels, pass), stream);
        if (e != hipSuccess) return e;
        have = out;
        out = out == s.permSorted ? s.perm : s.permSorted;
    }
    return launch_raysort_reorder(s.inRays, s.inSlotToId, n, have, 1, s.outRays, s.outIdToSlot, s.outSlotToId, stream);
}

}  // namespace mrt
