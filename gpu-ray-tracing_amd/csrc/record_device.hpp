// record_device.hpp — how the frame stages' kernels move their records (device only): a ray and a
// guide as two 16-byte halves, a colour as one, and the prologue of a kernel that runs one lane per
// primary slot. Inline helpers only; the records themselves are raygen_common.hpp's and
// denoise_common.hpp's, shared with the host.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "denoise_common.hpp"

namespace mrt {

__device__ inline rg::RayRec load_ray(const rg::RayRec* rays, int64_t at) {
    const float4* r = reinterpret_cast<const float4*>(rays + at);
    const float4 lo = r[0], hi = r[1];
    return rg::RayRec{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

__device__ inline void store_ray(rg::RayRec* out, int64_t at, const rg::RayRec& r) {
    float4* o = reinterpret_cast<float4*>(out + at);
    o[0] = make_float4(r.ox, r.oy, r.oz, r.tmin);
    o[1] = make_float4(r.dx, r.dy, r.dz, r.tmax);
}

__device__ inline denoise::Guide as_guide(const float4& lo, const float4& hi) {
    return denoise::Guide{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

__device__ inline denoise::Guide load_guide(const float4* guide, int q) {
    return as_guide(guide[2 * (int64_t)q], guide[2 * (int64_t)q + 1]);
}

__device__ inline denoise::Color as_color(const float4& v) { return denoise::Color{v.x, v.y, v.z, v.w}; }
__device__ inline float4 as_float4(const denoise::Color& c) { return make_float4(c.r, c.g, c.b, c.a); }

// What a lane that owns primary slot i starts from: the pixel the slot names, its ray, and the hit
// id and distance of its result.
struct PrimarySlot {
    int32_t pixel;
    rg::RayRec ray;
    int32_t id;
    float t;
};

// False where i is past the slots or the slot names no pixel of the frame: the lane has nothing to do.
__device__ inline bool load_primary_slot(int i, int numPrimary, const int32_t* slotToId, int numPixels,
                                         const rg::RayRec* rays, const int4* results, PrimarySlot& s) {
    if (i >= numPrimary) return false;
    s.pixel = slotToId[i];
    if (s.pixel < 0 || s.pixel >= numPixels) return false;
    s.ray = load_ray(rays, i);
    const int4 res = results[i];
    s.id = res.x;
    s.t = __int_as_float(res.y);
    return true;
}

}  // namespace mrt
