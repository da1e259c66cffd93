// light_common.hpp — an area light's shadow rays and the direct lighting they reconstruct, stated
// once for the host (csrc/host/light.cpp, g++) and the device (csrc/light_kernel.hip, hipcc), so
// that both give the same bits (the role scene_common.hpp has for the scene's attributes):
//   shadow_origin  the traced point backed off along its ray: o + d * max(t - 1e-4, 0), the
//                  framework's max, so a NaN t backs off by 0 (reference RayGenKernels.cu:252-253;
//                  the AO generator's origin, raygen_common.hpp)
//   shadow_offset  the Cranley-Patterson offset of one input ray: jenkinsMix twice over
//                  (seed + task, 0x9e3779b9, 0x9e3779b9), each word converted to float (round to
//                  nearest even: a word >= 0xFFFFFF80 converts to 2^32) times 2^-32, so an offset
//                  of exactly 1 exists (RayGenKernels.cu:257-262)
//   sobol2d        RayGenKernels.cu:54-75, with its `r2 ^= v2 << 1`
//   hammersley     (i + 0.5f) / n (RayGenKernels.cu:49-52)
//   shadow_pos     (sobol.x, sobol.y, hammersley) + offset, `if (p >= 1) p -= 1`, then p * 2, then
//                  - 1 (RayGenKernels.cu:271-276): a point of the cube [-1, 1)^3
//   shadow_ray     target = light + radius * pos, dir = target - origin, direction = dir * (1 *
//                  rcp(length)) with rcp(0) = 0 (VectorBase::normalized), tmin 0, tmax the length,
//                  or -1 where the input ray missed (id -1) (RayGenKernels.cu:280-291). A zero
//                  length gives a zero direction; so does an infinite one over finite components.
//                  No table is read: every id but -1 gives a live ray.
//   lit_factor     what one unblocked sample adds to a pixel: max(dot(nf, l), 0), l the unit vector
//                  from the backed-off point to the light's centre, nf the triangle's normal turned
//                  against the ray; the framework's max, so a NaN gives 0
//   lit_pixel      (material.xyz * (k * v), 1) as ABGR, v = unblocked / n
//   from_abgr / to_abgr  RendererKernels.cu:38-56, the device variant: truncating
// Both sides are built with -ffp-contract=off; the device file without denormal flushing and with
// correctly rounded division and square root (Makefile), so every float is the IEEE value on both
// sides. Only the bits of a NaN that an operation makes differ (x86 0xFFC00000, gfx950 0x7FC00000).
#pragma once
#include <cmath>
#include <cstdint>

#include "raygen_common.hpp"
#include "scene_common.hpp"

namespace mrt {
namespace light {

using scene::dot3;
using scene::normalize3;

constexpr float kEpsilon = 1.0e-4f;

MRT_HD inline void shadow_origin(const rg::RayRec& in, float t, float origin[3]) {
    const float back = woop::fw_max(t - kEpsilon, 0.0f);
    origin[0] = in.ox + in.dx * back;
    origin[1] = in.oy + in.dy * back;
    origin[2] = in.oz + in.dz * back;
}

MRT_HD inline void shadow_offset(uint32_t seed, uint32_t task, float offset[3]) {
    uint32_t a = seed + task, b = 0x9e3779b9u, c = 0x9e3779b9u;
    rg::jenkins_mix(a, b, c);
    rg::jenkins_mix(a, b, c);
    offset[0] = (float)a * 0x1p-32f;
    offset[1] = (float)b * 0x1p-32f;
    offset[2] = (float)c * 0x1p-32f;
}

MRT_HD inline void sobol2d(int i, float out[2]) {
    uint32_t r1 = 0, r2 = 0;
    for (uint32_t v1 = 1u << 31, v2 = 3u << 30; i; i >>= 1) {
        if (i & 1) {
            r1 ^= v1;
            r2 ^= v2 << 1;
        }
        v1 |= v1 >> 1;
        v2 ^= v2 >> 1;
    }
    out[0] = (float)r1 * 0x1p-32f;
    out[1] = (float)r2 * 0x1p-32f;
}

MRT_HD inline float hammersley(int i, int n) { return ((float)i + 0.5f) / (float)n; }

MRT_HD inline void shadow_pos(int i, int n, const float offset[3], float pos[3]) {
    float s[2];
    sobol2d(i, s);
    const float q[3] = {s[0], s[1], hammersley(i, n)};
    for (int k = 0; k < 3; k++) {
        float p = q[k] + offset[k];
        if (p >= 1.0f) p -= 1.0f;
        p = p * 2.0f;
        pos[k] = p - 1.0f;
    }
}

MRT_HD inline rg::RayRec shadow_ray(const float origin[3], const float offset[3], int32_t id, int i, int n,
                                    const float lightPos[3], float radius) {
    float pos[3], dir[3];
    shadow_pos(i, n, offset, pos);
    for (int k = 0; k < 3; k++) {
        const float target = lightPos[k] + radius * pos[k];
        dir[k] = target - origin[k];
    }
    const float len = sqrtf(dot3(dir, dir));
    const float s = 1.0f * woop::fw_rcp(len);
    return rg::RayRec{origin[0], origin[1], origin[2], 0.0f, dir[0] * s, dir[1] * s, dir[2] * s, id == -1 ? -1.0f : len};
}

// Sample i of n for input ray `task` of its batch: everything above in one call.
MRT_HD inline rg::RayRec shadow_sample(const rg::RayRec& in, int32_t id, float t, uint32_t seed, uint32_t task, int i,
                                       int n, const float lightPos[3], float radius) {
    float origin[3], offset[3];
    shadow_origin(in, t, origin);
    shadow_offset(seed, task, offset);
    return shadow_ray(origin, offset, id, i, n, lightPos, radius);
}

MRT_HD inline float lit_factor(const rg::RayRec& in, float t, const float normal[3], const float lightPos[3]) {
    float origin[3], l[3];
    shadow_origin(in, t, origin);
    const float toLight[3] = {lightPos[0] - origin[0], lightPos[1] - origin[1], lightPos[2] - origin[2]};
    normalize3(toLight, l);
    const float d[3] = {in.dx, in.dy, in.dz};
    float nf[3] = {normal[0], normal[1], normal[2]};
    if (dot3(nf, d) > 0.0f) {
        nf[0] = -nf[0];
        nf[1] = -nf[1];
        nf[2] = -nf[2];
    }
    const float c = dot3(nf, l);
    return c > 0.0f ? c : 0.0f;
}

MRT_HD inline void from_abgr(uint32_t c, float v[4]) {
    const float k = 1.0f / 255.0f;
    v[0] = (float)(c & 0xFF) * k;
    v[1] = (float)((c >> 8) & 0xFF) * k;
    v[2] = (float)((c >> 16) & 0xFF) * k;
    v[3] = (float)(c >> 24) * k;
}

MRT_HD inline uint32_t to_abgr(const float v[4]) {
    return (uint32_t)(fminf(fmaxf(v[0], 0.0f), 1.0f) * 255.0f) | ((uint32_t)(fminf(fmaxf(v[1], 0.0f), 1.0f) * 255.0f) << 8) |
           ((uint32_t)(fminf(fmaxf(v[2], 0.0f), 1.0f) * 255.0f) << 16) |
           ((uint32_t)(fminf(fmaxf(v[3], 0.0f), 1.0f) * 255.0f) << 24);
}

MRT_HD inline uint32_t background_pixel() {
    const float bg[4] = {0.2f, 0.4f, 0.8f, 1.0f};
    return to_abgr(bg);
}

// unblocked of the primary's n shadow rays missed (id -1): they reached their light samples.
MRT_HD inline uint32_t lit_pixel(uint32_t material, float k, int unblocked, int n) {
    const float v = (float)unblocked * (1.0f / (float)n);
    const float kv = k * v;
    float m[4];
    from_abgr(material, m);
    const float c[4] = {m[0] * kv, m[1] * kv, m[2] * kv, 1.0f};
    return to_abgr(c);
}

}  // namespace light
}  // namespace mrt
