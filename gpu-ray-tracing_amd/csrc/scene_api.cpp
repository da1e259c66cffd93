// scene_api.cpp — the C-ABI of what a moving scene needs beside its refitted tree:
// mrt_scene_attributes (the normals and colours the frame path reads, from device vertices) and
// mrt_tracer_tree_cost (the bound tree's area sums, for the caller's refit-or-rebuild decision).
// The argument checks and the launches (scene_kernel.hip). Both are enqueued on the caller's
// stream; only mrt_tracer_tree_cost with a host output waits, for its one readback.
#include "scene_common.hpp"
#include "scene_kernel.hpp"
#include "tracer.hpp"

using mrt::DeviceGuard;
using mrt::fail;
using mrt::hipFail;

static_assert(sizeof(mrt_tree_cost) == 64, "mrt_tree_cost is four doubles and four int64");

extern "C" {

int mrt_scene_attributes(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                         const float* triDiffuse, float* triNormals, uint32_t* triShadedColor,
                         uint32_t* triMaterialColor, int64_t* skipped, void* stream) {
    if (numVertices < 0 || numTriangles < 0) return fail(MRT_ERR_INVALID_ARG, "scene_attributes: negative count");
    if (!triNormals && !triShadedColor && !triMaterialColor)
        return fail(MRT_ERR_INVALID_ARG, "scene_attributes: no output");
    if (numTriangles == 0) return MRT_OK;
    if (!vertices || !triangles) return fail(MRT_ERR_INVALID_ARG, "scene_attributes: null vertices or triangles");
    if (numTriangles > mrt::scene::kMaxTriangles)
        return fail(MRT_ERR_TOO_LARGE, "scene_attributes: more than 67108863 triangles (the refit's limit)");
    mrt::SceneAttrArgs a{};
    a.vertices = vertices;
    a.numVertices = numVertices;
    a.triangles = triangles;
    a.numTriangles = (int)numTriangles;
    a.triDiffuse = triDiffuse;
    a.triNormals = triNormals;
    a.triShadedColor = triShadedColor;
    a.triMaterialColor = triMaterialColor;
    a.skipped = reinterpret_cast<unsigned long long*>(skipped);
    MRT_HIP(mrt::launch_scene_attributes(a, static_cast<hipStream_t>(stream)));
    return MRT_OK;
}

int mrt_tracer_tree_cost(mrt_tracer* t, mrt_tree_cost* host, void* device, void* stream) {
    if (!t) return fail(MRT_ERR_INVALID_ARG, "null tracer");
    if (!host && !device) return fail(MRT_ERR_INVALID_ARG, "tree_cost: no output");
    std::lock_guard<std::mutex> lock(t->mu);
    if (!t->bvh) return fail(MRT_ERR_NOT_BOUND, "tree_cost before bind (no BVH)");
    DeviceGuard guard(t->device);
    hipStream_t s = static_cast<hipStream_t>(stream);

    mrt::TreeCostArgs a{};
    a.nodes = static_cast<const uint32_t*>(t->bvh.nodes);
    a.numNodes = (int)t->bvh.numNodes();
    a.woop = static_cast<const uint32_t*>(t->bvh.woop);
    a.woopSlots = (int)(t->bvh.woopBytes / 16);
    if (a.numNodes <= 0) return fail(MRT_ERR_INVALID_ARG, "tree_cost: the bound tree has no record");
    const size_t partialBytes = (size_t)mrt::cost_partials(a.numNodes) * sizeof(mrt::CostPartial);
    mrt::StreamScratch scratch;
    if (hipError_t e = scratch.alloc(partialBytes + (device ? 0 : sizeof(mrt_tree_cost)), s))
        return hipFail(e, "hipMallocAsync(tree cost scratch)");
    a.partials = scratch.as<mrt::CostPartial>();
    a.out = device ? static_cast<mrt_tree_cost*>(device)
                   : reinterpret_cast<mrt_tree_cost*>(scratch.as<char>() + partialBytes);
    hipError_t e = mrt::launch_tree_cost(a, s);
    if (e == hipSuccess && host) e = hipMemcpyAsync(host, a.out, sizeof(mrt_tree_cost), hipMemcpyDeviceToHost, s);
    const hipError_t f = scratch.release();
    if (e != hipSuccess) return hipFail(e, "tree cost launch");
    if (f != hipSuccess) return hipFail(f, "hipFreeAsync(tree cost scratch)");
    if (host) MRT_HIP(hipStreamSynchronize(s));
    return MRT_OK;
}

}  // extern "C"
