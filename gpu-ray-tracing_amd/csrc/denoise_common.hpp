// denoise_common.hpp — the edge-avoiding a-trous wavelet filter of a path frame (Dammertz et al. 2010)
// and the features that guide it, stated once for the host (csrc/host/denoise.cpp, g++) and the
// device (csrc/denoise_kernel.hip, hipcc), so that both give the same bits (the role path_common.hpp
// has for the path step). include/mrt.h (mrt_denoise_features, mrt_denoise_filter) states the
// contract; here, term for term:
//   features_one   a primary slot's guide record {nf, hit flag, x, 0} and albedo from its ray, its
//                  result and the triangle tables
//   demodulate     image / albedo per channel where albedo > 0, else 0, at a hit; the image at a miss
//   tap_weight     ((h * a) * wz) * wc of one tap: a the clamped normal dot squared `squarings` times,
//                  wz = 1 / (1 + dpl^2) from the tap's distance to the centre's plane, wc = 1 / (1 +
//                  dc2 * invColor2) from the colour difference
//   filter_pixel   one pixel of one iteration: the 5x5 taps at `step`, dy outer and dx inner, both
//                  ascending; sum / wsum where wsum > 0, else the centre's colour
//   remodulate     c * albedo at a hit
// The taps come through a source object (guide(x, y), color(x, y, hit)), so the arithmetic does not
// know where a record is staged. Nothing here calls libm: the weights are rational, with no exp and no
// pow. Both sides are built with -ffp-contract=off; the device file without denormal flushing and
// with correctly rounded division (Makefile), so every float is the IEEE value on both sides. Only
// the bits of a NaN that an operation makes differ.
#pragma once
#include <cmath>
#include <cstdint>

#include "light_common.hpp"

namespace mrt {
namespace denoise {

// A pixel's guide: 32 bytes. hit != 0: the primary hit at x with the normal nf turned against the ray.
struct Guide {
    float nx, ny, nz, hit;
    float px, py, pz, pad;
};

struct Color {
    float r, g, b, a;
};

// The B3 spline's taps at |offset| 0, 1, 2; every product of two is exact.
MRT_HD inline float tap_h(int offset) {
    const int a = offset < 0 ? -offset : offset;
    return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}

MRT_HD inline bool is_hit(const Guide& g) { return g.hit != 0.0f; }

MRT_HD inline void features_one(const rg::RayRec& in, int32_t id, float t, const float* triNormals,
                                const uint32_t* triMaterialColor, int64_t numTris, Guide& g, Color& albedo) {
    if (!(id >= 0 && (int64_t)id < numTris)) {
        g = Guide{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        albedo = Color{1.0f, 1.0f, 1.0f, 1.0f};
        return;
    }
    const float* n = triNormals + 3 * (int64_t)id;
    rg::V3 nf = rg::make(n[0], n[1], n[2]);
    if (rg::dot(nf, rg::make(in.dx, in.dy, in.dz)) > 0.0f) nf = rg::neg(nf);
    g = Guide{nf.x, nf.y, nf.z, 1.0f, in.ox + in.dx * t, in.oy + in.dy * t, in.oz + in.dz * t, 0.0f};
    float a[4];
    light::from_abgr(triMaterialColor[id], a);
    albedo = Color{a[0], a[1], a[2], 1.0f};
}

MRT_HD inline float demodulate_channel(float image, float albedo) { return albedo > 0.0f ? image / albedo : 0.0f; }

MRT_HD inline Color demodulate(const Color& image, const Color& albedo, bool hit) {
    if (!hit) return image;
    return Color{demodulate_channel(image.r, albedo.r), demodulate_channel(image.g, albedo.g),
                 demodulate_channel(image.b, albedo.b), image.a};
}

MRT_HD inline Color remodulate(const Color& c, const Color& albedo, bool hit) {
    if (!hit) return c;
    return Color{c.r * albedo.r, c.g * albedo.g, c.b * albedo.b, c.a};
}

MRT_HD inline float tap_weight(const Guide& gp, const Guide& gq, const Color& cp, const Color& cq, float hw, float invPlane,
                               float invColor2, int squarings) {
    const rg::V3 np = rg::make(gp.nx, gp.ny, gp.nz);
    float a = rg::dot(np, rg::make(gq.nx, gq.ny, gq.nz));
    a = (a > 0.0f) ? a : 0.0f;
    for (int i = 0; i < squarings; i++) a = a * a;
    const float dpl = rg::dot(np, rg::make(gq.px - gp.px, gq.py - gp.py, gq.pz - gp.pz)) * invPlane;
    const float wz = 1.0f / (1.0f + dpl * dpl);
    const float ex = cq.r - cp.r, ey = cq.g - cp.g, ez = cq.b - cp.b;
    const float dc2 = ex * ex + ey * ey + ez * ez;
    const float wc = 1.0f / (1.0f + dc2 * invColor2);
    return ((hw * a) * wz) * wc;
}

// c_{k+1}(x, y) from c_k through src: src.guide(qx, qy) is a pixel's guide, src.color(qx, qy, hit) its c_k.
template <class Src>
MRT_HD inline Color filter_pixel(const Src& src, int x, int y, int width, int height, int step, float invPlane,
                                 float invColor2, int squarings) {
    const Guide gp = src.guide(x, y);
    const Color cp = src.color(x, y, is_hit(gp));
    if (!is_hit(gp)) return cp;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= width) continue;
            const Guide gq = src.guide(qx, qy);
            if (!is_hit(gq)) continue;
            const Color cq = src.color(qx, qy, true);
            const float w = tap_weight(gp, gq, cp, cq, tap_h(dx) * tap_h(dy), invPlane, invColor2, squarings);
            sr += w * cq.r;
            sg += w * cq.g;
            sb += w * cq.b;
            wsum += w;
        }
    }
    if (wsum > 0.0f) return Color{sr / wsum, sg / wsum, sb / wsum, cp.a};
    return cp;
}

// The written pixel: (r, 1) through the truncating device toABGR, as mrt_path_resolve's.
MRT_HD inline uint32_t pixel_of(const Color& r) {
    const float v[4] = {r.r, r.g, r.b, 1.0f};
    return light::to_abgr(v);
}

}  // namespace denoise
}  // namespace mrt
