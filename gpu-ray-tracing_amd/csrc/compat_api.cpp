// compat_api.cpp — the implicit per-device tracers (mrt_bind_bvh / mrt_unbind_bvh /
// mrt_trace) and the reference-compatible entry points of CudaTracerKernels.hh:42-52,
// RayGenKernels.hh, RendererKernels.hh and RayBufferKernels.hh:112-117, written against the public
// mrt_* functions of include/mrt.h (the three steps of the ray sort, which mrt_ray_sort runs as one
// call, through raysort_kernel.hpp's launches).
#include <climits>

#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "api_common.hpp"
#include "raysort_kernel.hpp"

using mrt::fail;
using mrt::hipFail;

namespace {

// ---- implicit per-device tracers (convenience + reference-compat API) ----
constexpr int kMaxDevices = 64;
std::mutex g_devMu;
mrt_tracer* g_devTracer[kMaxDevices] = {};

mrt_tracer* device_tracer(int* err) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        *err = fail(MRT_ERR_NO_DEVICE, "no current HIP device");
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_devMu);
    if (!g_devTracer[dev]) {
        mrt_tracer* t = nullptr;
        *err = mrt_tracer_create(dev, &t);
        if (*err) return nullptr;
        g_devTracer[dev] = t;
    }
    *err = MRT_OK;
    return g_devTracer[dev];
}

// cutilSafeCall-style fatal error for the compat entry points
// (reference cutil_inline_runtime.h:32-42).
void compat_check(int rc, const char* file, int line) {
    if (rc != MRT_OK) {
        std::fprintf(stderr, "[%s,%d] (HIP error %d: %s)\n", file, line, rc, mrt_last_error_detail());
        std::exit(-1);
    }
}

}  // namespace

extern "C" {

int mrt_bind_bvh(const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                 const int32_t* triIndex, int64_t triIndexBytes) {
    int err = 0;
    mrt_tracer* t = device_tracer(&err);
    if (!t) return err;
    return mrt_tracer_bind(t, nodes, nodeBytes, woop, woopBytes, triIndex, triIndexBytes);
}

int mrt_unbind_bvh(void) {
    int err = 0;
    mrt_tracer* t = device_tracer(&err);
    if (!t) return err;
    return mrt_tracer_unbind(t);
}

int mrt_trace(const void* rays, void* results, int32_t numRays, int32_t anyHit, void* stream, float* outMs) {
    int err = 0;
    mrt_tracer* t = device_tracer(&err);
    if (!t) return err;
    const uint32_t flags = anyHit ? MRT_TRACE_ANY_HIT : 0u;
    if (!outMs) return mrt_tracer_trace(t, rays, results, numRays, flags, nullptr, stream);
    mrt_trace_info info;
    const int rc = mrt_tracer_trace_timed(t, rays, results, numRays, flags, nullptr, stream, &info);
    *outMs = info.kernel_ms;
    return rc;
}

// ---- reference-compatible entry points --------------------------------------

void bind_CudaBVHTexture(void* nodeBuf, int64_t nodeBufSize, void* triWoopBuf, int64_t triWoopSize,
                         int32_t* triIndexBuf, int64_t triIndexSize) {
    compat_check(mrt_bind_bvh(nodeBuf, nodeBufSize, triWoopBuf, triWoopSize, triIndexBuf, triIndexSize), __FILE__,
                 __LINE__);
}

void unbind_CudaBVHTexture(void) { compat_check(mrt_unbind_bvh(), __FILE__, __LINE__); }

float launch_tracingKernel(int32_t nthreads, int32_t* blockSize, int numRays, bool anyHit, void* rays,
                           void* results, void* nodesA, void* nodesB, void* nodesC, void* nodesD, void* trisA,
                           void* trisB, void* trisC, int32_t* triIndices) {
    // The reference ignored nthreads/blockSize (CudaKernel::setGrid rewrote
    // them) and read the BVH through the textures bound earlier; the node/tri
    // pointers are accepted for ABI compatibility only.
    (void)nthreads; (void)blockSize; (void)nodesA; (void)nodesB; (void)nodesC; (void)nodesD;
    (void)trisA; (void)trisB; (void)trisC; (void)triIndices;
    float ms = 0.0f;
    compat_check(mrt_trace(rays, results, numRays, anyHit ? 1 : 0, nullptr, &ms), __FILE__, __LINE__);
    return ms;
}

void copy_tracing_results(void* result_host, void* result_dev, int32_t size) {
    const hipError_t e = hipMemcpy(result_host, result_dev, (size_t)size * 16u, hipMemcpyDeviceToHost);
    if (e != hipSuccess) compat_check(hipFail(e, "hipMemcpy"), __FILE__, __LINE__);
}

void launch_rayGenPrimaryKernel(int32_t nthreads, mrt_raygen_primary_input* in) {
    (void)nthreads;
    if (!in) compat_check(fail(MRT_ERR_INVALID_ARG, "null RayGenPrimaryInput"), __FILE__, __LINE__);
    compat_check(mrt_raygen_primary(in->nscreenToWorld, in->origin, in->maxDist, in->w, in->h, in->indexToPixel,
                                    in->rays, in->slotToID, in->idToSlot, nullptr),
                 __FILE__, __LINE__);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) compat_check(hipFail(e, "hipDeviceSynchronize"), __FILE__, __LINE__);
}

void launch_rayGenAOKernel(int32_t nthreads, mrt_raygen_ao_input* in) {
    (void)nthreads;
    if (!in || in->firstInputSlot < 0)
        compat_check(fail(MRT_ERR_INVALID_ARG, "bad RayGenAOInput"), __FILE__, __LINE__);
    // inSlot = taskIdx + firstInputSlot; the hash and the output slots use taskIdx (RayGenKernels.cu:128-131,163)
    const char* inRays = static_cast<const char*>(in->inRays);
    const char* inResults = static_cast<const char*>(in->inResults);
    compat_check(mrt_raygen_ao(inRays ? inRays + (int64_t)in->firstInputSlot * 32 : nullptr,
                               inResults ? inResults + (int64_t)in->firstInputSlot * 16 : nullptr, in->numInputRays,
                               static_cast<const float*>(in->normals), INT64_MAX, in->numSamples, in->maxDist,
                               in->randomSeed, in->outRays, in->outIDToSlot, in->outSlotToID, nullptr),
                 __FILE__, __LINE__);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) compat_check(hipFail(e, "hipDeviceSynchronize"), __FILE__, __LINE__);
}

void launch_reconstructKernel(int32_t nthreads, mrt_reconstruct_input* in) {
    (void)nthreads;   // the reference's CudaKernel::setGrid(nthreads) shape; ours is fixed
    if (!in) compat_check(fail(MRT_ERR_INVALID_ARG, "null ReconstructInput"), __FILE__, __LINE__);
    const int32_t type = in->isAO ? MRT_RAY_AO : (in->isDiffuse ? MRT_RAY_DIFFUSE : MRT_RAY_PRIMARY);
    compat_check(mrt_reconstruct(type, in->numRaysPerPrimary, in->firstPrimary, in->numPrimary, in->primarySlotToID,
                                 in->primaryResults, in->batchIDToSlot, in->batchResults, in->triMaterialColor,
                                 in->triShadedColor, in->pixels, nullptr),
                 __FILE__, __LINE__);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) compat_check(hipFail(e, "hipDeviceSynchronize"), __FILE__, __LINE__);
}

int32_t launch_countHitsKernel(int32_t threads, const int32_t* blockSize, mrt_count_hits_input* in) {
    (void)threads; (void)blockSize;   // launch shape of the reference (RendererKernels.cu:191-199)
    if (!in) compat_check(fail(MRT_ERR_INVALID_ARG, "null CountHitsInput"), __FILE__, __LINE__);
    int32_t* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(int32_t));
    if (e != hipSuccess) compat_check(hipFail(e, "hipMalloc"), __FILE__, __LINE__);
    compat_check(mrt_count_hits(in->rayResults, in->numRays, d, nullptr), __FILE__, __LINE__);
    int32_t n = 0;
    e = hipMemcpy(&n, d, sizeof(int32_t), hipMemcpyDeviceToHost);
    const hipError_t f = hipFree(d);
    if (e != hipSuccess) compat_check(hipFail(e, "hipMemcpy"), __FILE__, __LINE__);
    if (f != hipSuccess) compat_check(hipFail(f, "hipFree"), __FILE__, __LINE__);
    return n;
}

// ---- RayBufferKernels.hh:112-117 (RayBuffer::mortonSort's three launches) ----

void launch_findAABBKernel(int32_t nthreads, const int32_t* blockSize, mrt_find_aabb_input* in,
                           mrt_find_aabb_output* out) {
    (void)nthreads; (void)blockSize;   // launch shape of the reference (RayBuffer.cc:267-268)
    if (!in || !out || in->numRays < 0 || in->numRays > mrt::raysort::kMaxRays || (in->numRays > 0 && !in->inRays))
        compat_check(fail(MRT_ERR_INVALID_ARG, "bad FindAABBInput"), __FILE__, __LINE__);
    if (in->numRays == 0) return;      // the reference's one block returns at once
    mrt::DeviceBuf<float> scratch;     // the partials, then the box
    hipError_t e = scratch.alloc((size_t)(mrt::kRaySortBoxBlocks + 1) * 6 * sizeof(float));
    if (e != hipSuccess) compat_check(hipFail(e, "hipMalloc"), __FILE__, __LINE__);
    float* box = scratch.get() + (size_t)mrt::kRaySortBoxBlocks * 6;
    e = mrt::launch_raysort_box(static_cast<const uint4*>(in->inRays), in->numRays, 0, scratch.get(), box, nullptr);
    if (e != hipSuccess) compat_check(hipFail(e, "find AABB launch"), __FILE__, __LINE__);
    float got[6];
    e = hipMemcpy(got, box, sizeof(got), hipMemcpyDeviceToHost);
    if (e != hipSuccess) compat_check(hipFail(e, "hipMemcpy"), __FILE__, __LINE__);
    // the reference's atomicMin / atomicMax into the caller's box
    mrt::raysort::Box all{{out->aabbLo[0], out->aabbLo[1], out->aabbLo[2]}, {out->aabbHi[0], out->aabbHi[1], out->aabbHi[2]}};
    mrt::raysort::box_merge(all, mrt::raysort::Box{{got[0], got[1], got[2]}, {got[3], got[4], got[5]}});
    for (int k = 0; k < 3; k++) {
        out->aabbLo[k] = all.lo[k];
        out->aabbHi[k] = all.hi[k];
    }
    e = hipDeviceSynchronize();
    if (e != hipSuccess) compat_check(hipFail(e, "hipDeviceSynchronize"), __FILE__, __LINE__);
}

void launch_genMortonKeysKernel(int32_t nthreads, const int32_t* blockSize, mrt_gen_morton_keys_input* in) {
    (void)nthreads; (void)blockSize;
    if (!in || in->numRays < 0 || in->numRays > mrt::raysort::kMaxRays || (in->numRays > 0 && (!in->inRays || !in->outKeys)))
        compat_check(fail(MRT_ERR_INVALID_ARG, "bad GenMortonKeysInput"), __FILE__, __LINE__);
    if (in->numRays == 0) return;
    static_assert(sizeof(mrt_morton_key) == 4 * (mrt::raysort::kKeyWords + 1), "MortonKey is oldSlot and six words");
    const mrt::raysort::Box box{{in->aabbLo[0], in->aabbLo[1], in->aabbLo[2]}, {in->aabbHi[0], in->aabbHi[1], in->aabbHi[2]}};
    hipError_t e = mrt::launch_raysort_keys(static_cast<const uint4*>(in->inRays), in->numRays, nullptr, box,
                                            reinterpret_cast<uint32_t*>(in->outKeys), mrt::raysort::kKeyWords + 1, nullptr);
    if (e != hipSuccess) compat_check(hipFail(e, "gen Morton keys launch"), __FILE__, __LINE__);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) compat_check(hipFail(e, "hipDeviceSynchronize"), __FILE__, __LINE__);
}

void launch_reorderRaysKernel(int32_t nthreads, mrt_reorder_rays_input* in) {
    (void)nthreads;
    if (!in || in->numRays < 0 || in->numRays > mrt::raysort::kMaxRays ||
        (in->numRays > 0 && (!in->inKeys || !in->inRays || !in->outRays)))
        compat_check(fail(MRT_ERR_INVALID_ARG, "bad ReorderRaysInput"), __FILE__, __LINE__);
    if (in->numRays == 0) return;
    hipError_t e = mrt::launch_raysort_reorder(static_cast<const uint4*>(in->inRays), in->inSlotToID, in->numRays,
                                               &in->inKeys->oldSlot, mrt::raysort::kKeyWords + 1,
                                               static_cast<uint4*>(in->outRays), in->outIDToSlot, in->outSlotToID, nullptr);
    if (e != hipSuccess) compat_check(hipFail(e, "reorder rays launch"), __FILE__, __LINE__);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) compat_check(hipFail(e, "hipDeviceSynchronize"), __FILE__, __LINE__);
}

}  // extern "C"
