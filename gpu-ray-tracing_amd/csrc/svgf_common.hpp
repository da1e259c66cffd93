// svgf_common.hpp — variance-guided filtering of accumulated path frames (Schied et al. 2017): the
// temporal accumulation with the luminance moments carried along, the variance of a pixel from its
// moments or from its neighbours', and one iteration of the a-trous filter whose colour weight is
// scaled by that variance. Stated once for the host (csrc/host/svgf.cpp, g++) and the device
// (csrc/svgf_kernel.hip, hipcc), so that both give the same bits (the role temporal_common.hpp has
// for the accumulation). include/mrt_svgf.h states the contract; here, term for term:
//   accumulate_pixel  temporal::accumulate_pixel's steps with the moments: the same reprojection runs
//                     a second time over a source whose prev_history is the moments record, so the
//                     taps, their bw and wsum are the colour's
//   variance_pixel    c_0: the demodulated colour with pos(m2 - m1^2) in w, or the 7 x 7 estimate
//                     scaled by 4 / N where the history is shorter than 4
//   filter_pixel      one pixel of one iteration: the 3 x 3 Gaussian of the adjacent variances, the
//                     5 x 5 taps at `step` weighted by ((hw * a) * wz) * wl, the colour by sum / wsum
//                     and the variance by sum(w^2 v) / wsum^2
// The buffers come through source objects, so the arithmetic does not know where a record is
// staged. The guide record, the demodulation rule and the B3 taps are denoise_common.hpp's, the
// reprojection temporal_common.hpp's; both are used and not edited. Nothing here calls libm. Both
// sides are built with -ffp-contract=off; the device file without denormal flushing and with
// correctly rounded division (Makefile).
#pragma once
#include <cstdint>

#include "temporal_common.hpp"

namespace mrt {
namespace svgf {

using denoise::Color;
using denoise::Guide;

MRT_HD inline float lum(const Color& c) { return rg::dot(rg::make(0.2126f, 0.7152f, 0.0722f), rg::make(c.r, c.g, c.b)); }
MRT_HD inline float pos(float x) { return (x > 0.0f) ? x : 0.0f; }

// tap_weight's normal term: the clamped dot, squared `squarings` times.
MRT_HD inline float normal_term(const Guide& gp, const Guide& gq, int squarings) {
    float a = rg::dot(rg::make(gp.nx, gp.ny, gp.nz), rg::make(gq.nx, gq.ny, gq.nz));
    a = (a > 0.0f) ? a : 0.0f;
    for (int i = 0; i < squarings; i++) a = a * a;
    return a;
}

// tap_weight's plane term.
MRT_HD inline float plane_term(const Guide& gp, const Guide& gq, float invPlane) {
    const float dpl = rg::dot(rg::make(gp.nx, gp.ny, gp.nz), rg::make(gq.px - gp.px, gq.py - gp.py, gq.pz - gp.pz)) * invPlane;
    return 1.0f / (1.0f + dpl * dpl);
}

// A temporal source whose history is another record: reproject() then gathers that record over the
// taps, the bw and the wsum it gathers the colour history over.
template <class Src>
struct MomentsOf {
    const Src& src;
    MRT_HD Color prev_position(int p) const { return src.prev_position(p); }
    MRT_HD Guide prev_guide(int q) const { return src.prev_guide(q); }
    MRT_HD Color prev_history(int q) const { return src.prev_moments(q); }
};

// One pixel of mrt_svgf_accumulate. `history` and `result` are temporal::accumulate_pixel's.
template <class Src>
MRT_HD inline void accumulate_pixel(const Src& src, const temporal::Constants& k, int p, Color& history, Color& moments,
                                    Color& result) {
    const Guide gp = src.guide(p);
    const bool hit = denoise::is_hit(gp);
    const Color image = src.image(p);
    const Color albedo = hit ? src.albedo(p) : Color{1.0f, 1.0f, 1.0f, 1.0f};
    const Color c = denoise::demodulate(image, albedo, hit);
    const float l = lum(c), l2 = l * l;
    history = Color{c.r, c.g, c.b, 1.0f};
    moments = Color{l, l2, 0.0f, 1.0f};
    Color hst, hm;
    if (hit && k.havePrev && temporal::reproject(src, k, p, gp, hst) && temporal::reproject(MomentsOf<Src>{src}, k, p, gp, hm)) {
        const float n1 = hst.a + 1.0f;
        const float N = (n1 < (float)k.maxHistory) ? n1 : (float)k.maxHistory;
        const float alpha = 1.0f / N;
        history = Color{hst.r + (c.r - hst.r) * alpha, hst.g + (c.g - hst.g) * alpha, hst.b + (c.b - hst.b) * alpha, N};
        moments = Color{hm.r + (l - hm.r) * alpha, hm.g + (l2 - hm.g) * alpha, 0.0f, N};
    }
    result = denoise::remodulate(Color{history.r, history.g, history.b, image.a}, albedo, hit);
}

constexpr float kShortHistory = 4.0f;   // below it the variance comes from the neighbours' moments
constexpr int kVarianceRadius = 3;      // of the 7 x 7 window

// c_0 of a pixel: src.guide(x, y), src.image(x, y) (the accumulated frame's), src.albedo(x, y),
// src.moments(x, y).
template <class Src>
MRT_HD inline Color variance_pixel(const Src& src, int x, int y, int width, int height, float invPlane, int squarings) {
    const Guide gp = src.guide(x, y);
    const Color image = src.image(x, y);
    if (!denoise::is_hit(gp)) return Color{image.r, image.g, image.b, 0.0f};
    const Color c = denoise::demodulate(image, src.albedo(x, y), true);
    const Color m = src.moments(x, y);
    const float own = pos(m.g - m.r * m.r);
    if (m.a >= kShortHistory) return Color{c.r, c.g, c.b, own};
    float s1 = 0.0f, s2 = 0.0f, wsum = 0.0f;
    for (int dy = -kVarianceRadius; dy <= kVarianceRadius; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -kVarianceRadius; dx <= kVarianceRadius; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= width) continue;
            const Guide gq = src.guide(qx, qy);
            if (!denoise::is_hit(gq)) continue;
            const Color mq = src.moments(qx, qy);
            const float w = normal_term(gp, gq, squarings) * plane_term(gp, gq, invPlane);
            s1 += w * mq.r;
            s2 += w * mq.g;
            wsum += w;
        }
    }
    const float scale = 4.0f / m.a;
    if (wsum > 0.0f) {
        const float M1 = s1 / wsum, M2 = s2 / wsum;
        return Color{c.r, c.g, c.b, pos(M2 - M1 * M1) * scale};
    }
    return Color{c.r, c.g, c.b, own * scale};
}

// The 3 x 3 Gaussian's taps at |dx| + |dy| = 0, 1, 2.
MRT_HD inline float tap_g(int dx, int dy) {
    const int n = (dx != 0) + (dy != 0);
    return n == 0 ? 0.25f : (n == 1 ? 0.125f : 0.0625f);
}

// c_{k+1}(x, y) from c_k: src.guide(qx, qy) and src.color(qx, qy) are a tap's guide and c_k (w: the
// variance); src.near_hit(qx, qy) and src.near_variance(qx, qy) those of an adjacent pixel, which a
// tile staged a step apart does not hold.
template <class Src>
MRT_HD inline Color filter_pixel(const Src& src, int x, int y, int width, int height, int step, float invPlane,
                                 float sigmaLum2, int squarings) {
    const Guide gp = src.guide(x, y);
    const Color cp = src.color(x, y);
    if (!denoise::is_hit(gp)) return cp;
    float gs = 0.0f, gv = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= width) continue;
            if (!src.near_hit(qx, qy)) continue;
            const float g = tap_g(dx, dy);
            gv += g * src.near_variance(qx, qy);
            gs += g;
        }
    }
    const float vt = (gs > 0.0f) ? gv / gs : cp.a;
    const float invL = 1.0f / (sigmaLum2 * vt + 1e-8f);
    const float lp = lum(cp);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, wsum = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= width) continue;
            const Guide gq = src.guide(qx, qy);
            if (!denoise::is_hit(gq)) continue;
            const Color cq = src.color(qx, qy);
            const float hw = denoise::tap_h(dx) * denoise::tap_h(dy);
            const float dl = lum(cq) - lp;
            const float wl = 1.0f / (1.0f + (dl * dl) * invL);
            const float w = ((hw * normal_term(gp, gq, squarings)) * plane_term(gp, gq, invPlane)) * wl;
            sr += w * cq.r;
            sg += w * cq.g;
            sb += w * cq.b;
            sv += (w * w) * cq.a;
            wsum += w;
        }
    }
    if (wsum > 0.0f) return Color{sr / wsum, sg / wsum, sb / wsum, sv / (wsum * wsum)};
    return cp;
}

}  // namespace svgf
}  // namespace mrt
