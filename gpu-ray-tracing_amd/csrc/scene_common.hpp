// scene_common.hpp — what depends on vertex positions outside the BVH, stated once for the host
// (csrc/host/scene.cpp, host_api.cpp, g++) and the device (csrc/scene_kernel.hip, hipcc), so that
// both give the same bits (the role woop_common.hpp has for the refit):
//   tri_normal   Scene::Scene's face normal (reference Scene.cc:66-75):
//                normalize(cross(v1 - v0, v2 - v0)), normalize being a * (1 * rcp(length(a))) with
//                rcp(0) = 0 (Math.hh:113, VectorBase::normalized) and the dot product summed from 0
//   light_dir    normalize(1, 2, 3), the direction the shaded colour is lit from (Scene.cc:37)
//   shade        diffuse.xyz * (dot(n, light) * 0.5 + 0.5), alpha 1 (Scene.cc:75-80)
//   to_abgr      Vec4f::toABGR, host variant (Math.cc:45-52): clamp, scale by 2^56 in double, times
//                255, round half up in fixed point. The clamp is the framework's min(max(v, 0), 1)
//                with max(a, b) = a > b ? a : b (Defs.hh:141-159), which sends a NaN channel (the
//                shade of a triangle whose normal overflowed) to 0, not through.
//   tree_cost_term  the area one child slot of a Compact2 record adds to mrt_tree_cost: half the
//                surface area dx*dy + dy*dz + dz*dx, differences and products in double from the
//                float32 planes; not counted (skipped) when it is not finite or the box is inverted
// Both sides are built with -ffp-contract=off; the device file without denormal flushing and with
// correctly rounded division and square root (Makefile), so every float is the IEEE value on both
// sides. Only the bits of a NaN that an operation makes differ (x86 0xFFC00000, gfx950 0x7FC00000).
#pragma once
#include <cmath>
#include <cstdint>

#include "woop_common.hpp"

namespace mrt {
namespace scene {

constexpr int64_t kMaxTriangles = (((int64_t)1 << 28) - 2) / 4;   // the refit's and the build's (lbvh_common.hpp)

MRT_HD inline float dot3(const float a[3], const float b[3]) {   // VectorBase::dot: r = 0; r += a[i] * b[i]
    float r = 0.0f;
    r += a[0] * b[0];
    r += a[1] * b[1];
    r += a[2] * b[2];
    return r;
}

MRT_HD inline void normalize3(const float a[3], float out[3]) {
    const float s = 1.0f * woop::fw_rcp(sqrtf(dot3(a, a)));
    out[0] = a[0] * s;
    out[1] = a[1] * s;
    out[2] = a[2] * s;
}

MRT_HD inline void tri_normal(const float v0[3], const float v1[3], const float v2[3], float n[3]) {
    const float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};   // Math.hh:338
    normalize3(c, n);
}

MRT_HD inline void light_dir(float l[3]) {
    const float d[3] = {1.0f, 2.0f, 3.0f};
    normalize3(d, l);
}

MRT_HD inline uint32_t to_abgr(const float v[4]) {
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const float lo = v[i] > 0.0f ? v[i] : 0.0f;
        const float c = lo < 1.0f ? lo : 1.0f;
        const uint64_t q = (uint64_t)((double)c * 72057594037927936.0);   // exp2(56)
        r |= (uint32_t)((((q * 255u) >> 55) + 1) >> 1) << (8 * i);
    }
    return r;
}

// MeshBase::Material's default diffuse (Mesh.hh:92).
MRT_HD inline void default_diffuse(float d[4]) {
    d[0] = 0.75f;
    d[1] = 0.75f;
    d[2] = 0.75f;
    d[3] = 1.0f;
}

MRT_HD inline uint32_t shade(const float n[3], const float light[3], const float diffuse[4]) {
    const float k = dot3(n, light) * 0.5f + 0.5f;
    const float c[4] = {diffuse[0] * k, diffuse[1] * k, diffuse[2] * k, 1.0f};
    return to_abgr(c);
}

// The term of one box: *area = its half surface area. False (the box is in no sum) when it is
// inverted on some axis or the area is not finite (a NaN or infinite plane).
MRT_HD inline bool tree_cost_term(const woop::Box& b, double* area) {
    const double dx = (double)b.hi[0] - (double)b.lo[0], dy = (double)b.hi[1] - (double)b.lo[1],
                 dz = (double)b.hi[2] - (double)b.lo[2];
    const double xy = dx * dy, yz = dy * dz, zx = dz * dx;
    const double a = (xy + yz) + zx;
    *area = a;
    if (!(b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2])) return false;
    return a - a == 0.0;   // finite
}

// A leaf's triangles: the walk from its first Woop slot in steps of three up to its terminator
// or the end of the array, as the refit walks it. z0(s): the bits of slot s's first word.
template <class Z0>
MRT_HD inline int64_t leaf_triangles(int32_t ref, int64_t woopSlots, Z0 z0) {
    int64_t count = 0;
    for (int64_t s = ~(int64_t)ref; s + 2 < woopSlots; s += 3) {
        if (z0(s) == woop::kTerminatorBits) break;
        count++;
    }
    return count;
}

}  // namespace scene
}  // namespace mrt
