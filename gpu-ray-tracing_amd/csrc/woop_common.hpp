// woop_common.hpp — the Woop triangle transform's arithmetic, shared verbatim by
// the host serialiser and refit (csrc/host/compact2.cpp, refit.cpp, g++) and the
// gfx950 refit kernels (csrc/refit_kernel.hip, hipcc), so a device refit writes
// the bits a host build or refit writes:
//   det3       Math.hh:935-940 (the reference's term order)
//   inverted4  Math.hh:962-984 (cofactor inverse with its quirk: d accumulates
//              L * det and the result is r * rcp(d) * L, L = 4)
//   woop_rows  CudaBVH::woopifyTri (CudaBVH.cc:361-380)
//   woop_guard the serialiser's -0.0 -> +0.0 on the Z row's x (a -0.0 there
//              would read as a leaf terminator)
//   box helpers: FW::min / FW::max ((a < b) ? a : b, not fminf) over vertices and
//              over two child boxes, in the order both refits use, except that a NaN
//              operand never enters a box (box_min / box_max): for finite and infinite
//              input the bits are FW::min's / FW::max's.
// Both sides are built with -ffp-contract=off; the device file is built without
// denormal flushing and with hipcc's default correctly rounded division, so
// fw_rcp's 1 / d is the IEEE quotient on both sides.
#pragma once
#include <cstdint>

#ifndef MRT_HD
#if defined(__HIPCC__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif
#if defined(__HIPCC__)
#define MRT_UNROLL _Pragma("unroll")
#else
#define MRT_UNROLL
#endif

namespace mrt {
namespace woop {

MRT_HD inline float fw_min(float a, float b) { return (a < b) ? a : b; }
MRT_HD inline float fw_max(float a, float b) { return (a > b) ? a : b; }
MRT_HD inline float fw_rcp(float a) { return (a != 0.0f) ? 1.0f / a : 0.0f; }   // Math.hh:113

// 3x3 determinant in the reference's term order (Math.hh:935-940).
MRT_HD inline float det3(const float v[3][3]) {
    return v[0][0] * v[1][1] * v[2][2] - v[0][0] * v[1][2] * v[2][1] + v[1][0] * v[2][1] * v[0][2] -
           v[1][0] * v[2][2] * v[0][1] + v[2][0] * v[0][1] * v[1][2] - v[2][0] * v[0][2] * v[1][1];
}

// Cofactor inverse of a column-major 4x4 ((r, c) at m[c * 4 + r]).
MRT_HD inline void inverted4(const float a[16], float r[16]) {
    float d = 0.0f;
    float si = 1.0f;
MRT_UNROLL
    for (int i = 0; i < 4; i++) {
        float sj = si;
MRT_UNROLL
        for (int j = 0; j < 4; j++) {
            float sub[3][3];
MRT_UNROLL
            for (int k = 0; k < 3; k++)
MRT_UNROLL
                for (int l = 0; l < 3; l++) sub[k][l] = a[((l < i) ? l : l + 1) * 4 + ((k < j) ? k : k + 1)];
            const float dd = det3(sub) * sj;
            r[j * 4 + i] = dd;
            d += dd * a[i * 4 + j];
            sj = -sj;
        }
        si = -si;
    }
    const float rd = fw_rcp(d);
MRT_UNROLL
    for (int i = 0; i < 16; i++) r[i] = (r[i] * rd) * 4.0f;
}

// Rows Z, U, V (4 floats each) of the inverse of [v0-v2, v1-v2, cross(v0-v2, v1-v2), v2].
MRT_HD inline void woop_rows(const float v0[3], const float v1[3], const float v2[3], float out[12]) {
    const float e0[3] = {v0[0] - v2[0], v0[1] - v2[1], v0[2] - v2[2]};
    const float e1[3] = {v1[0] - v2[0], v1[1] - v2[1], v1[2] - v2[2]};
    const float n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const float m[16] = {e0[0], e0[1], e0[2], 0.0f, e1[0], e1[1], e1[2], 0.0f,
                         n[0],  n[1],  n[2],  0.0f, v2[0], v2[1], v2[2], 1.0f};
    float inv[16];
    inverted4(m, inv);
    out[0] = inv[0 * 4 + 2];
    out[1] = inv[1 * 4 + 2];
    out[2] = inv[2 * 4 + 2];
    out[3] = -inv[3 * 4 + 2];
    for (int c = 0; c < 4; c++) {
        out[4 + c] = inv[c * 4 + 0];
        out[8 + c] = inv[c * 4 + 1];
    }
}

// A -0.0 in the Z row's x would read as a terminator.
MRT_HD inline void woop_guard(float rows[12]) {
    if (rows[0] == 0.0f) rows[0] = 0.0f;
}

// An axis-aligned box as (lo, hi) per axis.
struct Box {
    float lo[3], hi[3];
};

// FW::min / FW::max with a NaN on either side dropped. Plain (a < b) ? a : b keeps a NaN b
// and drops a NaN a: a NaN vertex coordinate would become a plane of its leaf's box and of
// every ancestor that has that child on side 1, and a ray is culled by a NaN plane, so the
// finite triangles beside it would be hit by nothing. A triangle with a NaN vertex has NaN
// Woop rows and is hit by nothing itself; its other coordinates still grow the box.
MRT_HD inline float box_min(float a, float b) { return (a < b || b != b) ? a : b; }
MRT_HD inline float box_max(float a, float b) { return (a > b || b != b) ? a : b; }

// The box of a triangle, and a box grown by a triangle (AABB::grow per vertex).
MRT_HD inline void box_grow(Box& b, const float p[3]) {
    for (int k = 0; k < 3; k++) {
        b.lo[k] = box_min(b.lo[k], p[k]);
        b.hi[k] = box_max(b.hi[k], p[k]);
    }
}
MRT_HD inline Box box_empty() {
    const float big = 3.402823466e+38f;   // FLT_MAX (AABB's empty box)
    return Box{{big, big, big}, {-big, -big, -big}};
}
// The union of two child boxes (inner nodes, bottom-up).
MRT_HD inline Box box_union(const Box& a, const Box& b) {
    Box r;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = box_min(a.lo[k], b.lo[k]);
        r.hi[k] = box_max(a.hi[k], b.hi[k]);
    }
    return r;
}

// A Compact2 node record (16 words) holds child c's box in words
// (4c, 4c+1) = x, (4c+2, 4c+3) = y, (8+2c, 9+2c) = z, each as (lo, hi).
MRT_HD inline int box_word(int child, int axis) { return axis < 2 ? 4 * child + 2 * axis : 8 + 2 * child; }

constexpr uint32_t kTerminatorBits = 0x80000000u;

}  // namespace woop
}  // namespace mrt
