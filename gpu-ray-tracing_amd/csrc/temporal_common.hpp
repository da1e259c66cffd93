// temporal_common.hpp — the temporal accumulation of path frames: where a primary hit's surface
// point was in the previous frame, and the running mean of the demodulated image over the history
// found there. Stated once for the host (csrc/host/temporal.cpp, g++) and the device
// (csrc/temporal_kernel.hip, hipcc), so that both give the same bits (the role denoise_common.hpp
// has for the filter). include/mrt_temporal.h (mrt_temporal_motion, mrt_temporal_accumulate) states
// the contract; here, term for term:
//   motion_one        a primary slot's previous position {q, 1} from its ray, its result, the
//                     triangle's current vertices (barycentrics of the hit point by five dot
//                     products) and its previous ones; {0, 0, 0, 0} at a miss
//   accumulate_pixel  one pixel: demodulate, reproject through the previous frame's
//                     world-to-screen matrix, gather the four bilinear taps that pass the normal and
//                     plane tests, blend with 1 / N, remodulate
// The buffers come through a source object (image(p), guide(p), albedo(p), prev_position(p),
// prev_guide(q), prev_history(q)), so the arithmetic does not know how a record is loaded. The
// guide record, the demodulation rule and the ABGR conversions are denoise_common.hpp's. The only
// libm call is floorf, which is exact. Both sides are built with -ffp-contract=off; the device file
// without denormal flushing and with correctly rounded division (Makefile), so every float is the
// IEEE value on both sides. Only the bits of a NaN that an operation makes differ.
#pragma once
#include <cmath>
#include <cstdint>

#include "denoise_common.hpp"

namespace mrt {
namespace temporal {

using denoise::Color;
using denoise::Guide;

// What accumulate_pixel reads besides the buffers.
struct Constants {
    int32_t width, height;
    int32_t havePrev, maxHistory;
    int32_t hasPrevPosition;
    float normalCos, invPlane;
    float m[16];         // the previous frame's world-to-screen matrix, column-major
    float subpixel[2];   // the previous frame's sample position inside a pixel
};

MRT_HD inline rg::V3 vertex(const float* vertices, int32_t index) {
    const float* v = vertices + 3 * (int64_t)index;
    return rg::make(v[0], v[1], v[2]);
}

MRT_HD inline Color motion_one(const rg::RayRec& in, int32_t id, float t, const int32_t* triangles, int64_t numTris,
                               const float* vertices, const float* prevVertices, int64_t numVertices) {
    const Color none{0.0f, 0.0f, 0.0f, 0.0f};
    if (!(id >= 0 && (int64_t)id < numTris)) return none;
    const int32_t* tri = triangles + 3 * (int64_t)id;
    const int32_t i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if (i0 < 0 || i0 >= numVertices || i1 < 0 || i1 >= numVertices || i2 < 0 || i2 >= numVertices) return none;
    const rg::V3 x = rg::make(in.ox + in.dx * t, in.oy + in.dy * t, in.oz + in.dz * t);
    const rg::V3 v0 = vertex(vertices, i0), v1 = vertex(vertices, i1), v2 = vertex(vertices, i2);
    const rg::V3 e0 = rg::sub(v1, v0), e1 = rg::sub(v2, v0), r = rg::sub(x, v0);
    const float d00 = rg::dot(e0, e0), d01 = rg::dot(e0, e1), d11 = rg::dot(e1, e1);
    const float d20 = rg::dot(r, e0), d21 = rg::dot(r, e1);
    const float den = d00 * d11 - d01 * d01;
    if (!(den > 0.0f)) return Color{x.x, x.y, x.z, 1.0f};   // a degenerate triangle, a NaN: the point stays
    const float b1 = (d11 * d20 - d01 * d21) / den;
    const float b2 = (d00 * d21 - d01 * d20) / den;
    const float b0 = (1.0f - b1) - b2;
    const rg::V3 q0 = vertex(prevVertices, i0), q1 = vertex(prevVertices, i1), q2 = vertex(prevVertices, i2);
    return Color{(q0.x * b0 + q1.x * b1) + q2.x * b2, (q0.y * b0 + q1.y * b1) + q2.y * b2,
                 (q0.z * b0 + q1.z * b1) + q2.z * b2, 1.0f};
}

// Row i of the previous frame's matrix times (xw, 1): from 0, left to right, as primary_ray sums.
MRT_HD inline float clip_row(const float* m, int i, const rg::V3& xw) {
    float r = 0.0f;
    r += m[i] * xw.x;
    r += m[4 + i] * xw.y;
    r += m[8 + i] * xw.z;
    r += m[12 + i] * 1.0f;
    return r;
}

// The history reprojected to the current pixel whose guide is gp: false where there is none.
template <class Src>
MRT_HD inline bool reproject(const Src& src, const Constants& k, int p, const Guide& gp, Color& hst) {
    rg::V3 xw = rg::make(gp.px, gp.py, gp.pz);
    if (k.hasPrevPosition) {
        const Color pp = src.prev_position(p);
        if (pp.a == 0.0f) return false;
        xw = rg::make(pp.r, pp.g, pp.b);
    }
    const float cx = clip_row(k.m, 0, xw), cy = clip_row(k.m, 1, xw), cw = clip_row(k.m, 3, xw);
    if (!(cw > 0.0f)) return false;
    const float sx = ((cx / cw + 1.0f) * 0.5f) * (float)k.width - k.subpixel[0];
    const float sy = ((cy / cw + 1.0f) * 0.5f) * (float)k.height - k.subpixel[1];
    if (!(sx > -1.0f && sx < (float)k.width && sy > -1.0f && sy < (float)k.height)) return false;   // a NaN lands here
    const float fx = floorf(sx), fy = floorf(sy);
    const int ix = (int)fx, iy = (int)fy;
    const float ax = sx - fx, ay = sy - fy;
    const rg::V3 np = rg::make(gp.nx, gp.ny, gp.nz);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, wsum = 0.0f;
    for (int j = 0; j < 2; j++) {
        const int qy = iy + j;
        if (qy < 0 || qy >= k.height) continue;
        for (int i = 0; i < 2; i++) {
            const int qx = ix + i;
            if (qx < 0 || qx >= k.width) continue;
            const float bw = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            if (bw == 0.0f) continue;
            const int q = qy * k.width + qx;
            const Guide gq = src.prev_guide(q);
            if (!denoise::is_hit(gq)) continue;
            const rg::V3 nq = rg::make(gq.nx, gq.ny, gq.nz);
            if (!(rg::dot(np, nq) >= k.normalCos)) continue;
            const float dpl = rg::dot(nq, rg::make(gq.px - xw.x, gq.py - xw.y, gq.pz - xw.z));
            if (!(fabsf(dpl) * k.invPlane <= 1.0f)) continue;
            const Color h = src.prev_history(q);
            sr += bw * h.r;
            sg += bw * h.g;
            sb += bw * h.b;
            sa += bw * h.a;
            wsum += bw;
        }
    }
    if (!(wsum > 0.0f)) return false;
    hst = Color{sr / wsum, sg / wsum, sb / wsum, sa / wsum};
    return true;
}

// One pixel: `history` is the demodulated running mean with its length in a, `result` the
// remodulated colour with the image's own a.
template <class Src>
MRT_HD inline void accumulate_pixel(const Src& src, const Constants& k, int p, Color& history, Color& result) {
    const Guide gp = src.guide(p);
    const bool hit = denoise::is_hit(gp);
    const Color image = src.image(p);
    const Color albedo = hit ? src.albedo(p) : Color{1.0f, 1.0f, 1.0f, 1.0f};
    const Color c = denoise::demodulate(image, albedo, hit);
    history = Color{c.r, c.g, c.b, 1.0f};
    Color hst;
    if (hit && k.havePrev && reproject(src, k, p, gp, hst)) {
        const float n1 = hst.a + 1.0f;
        const float N = (n1 < (float)k.maxHistory) ? n1 : (float)k.maxHistory;
        const float alpha = 1.0f / N;
        history = Color{hst.r + (c.r - hst.r) * alpha, hst.g + (c.g - hst.g) * alpha, hst.b + (c.b - hst.b) * alpha, N};
    }
    result = denoise::remodulate(Color{history.r, history.g, history.b, image.a}, albedo, hit);
}

}  // namespace temporal
}  // namespace mrt
