// path_common.hpp — one vertex of a Lambertian path with next-event estimation, its accumulation
// and the resolve of a batch's paths into pixels, stated once for the host (csrc/host/path.cpp,
// g++) and the device (csrc/path_kernel.hip, hipcc), so that both give the same bits (the role
// light_common.hpp has for the shadow frame). include/mrt.h (mrt_path_extend) states the contract;
// here, term for term:
//   hash_words    jenkins_mix twice over (seed + vertex * 0x9e3779b9 + key, 0x9e3779b9, 0x9e3779b9)
//                 gives the light sample's offset words; a third mix of the same three words gives
//                 the two words that shift the bounce's Halton point
//   halton23      the two radical-inverse loops ao_sample_xyz (raygen_common.hpp) runs before its
//                 warp, restated: base 2 over (unsigned)(s + 1), base 3 over s + 1
//   sincos_turn   cos and sin of 2*pi*u for u in [0, 1) with no libm call: v = 4u (exact),
//                 q = (int)v, f = v - q (exact), f > 0.5 moves to f - 1 and q + 1 (exact), so that
//                 |f| <= 0.5 of a quarter turn; sin(pi/2 f) and cos(pi/2 f) are a fixed odd degree-9
//                 and even degree-10 polynomial in f in Horner form (`+` and `*` only); q & 3 turns
//                 the pair by quarter turns
//   frame         ao_basis's perp / biperp of the normal, without its hash rotation
//   bounce_dir    r = sqrtf(u1), x = r cos, y = r sin, z = sqrtf(max(1 - x*x - y*y, 0)),
//                 normalize(t0 * x + t1 * y + nf * z)
//   extend        the whole vertex step of one slot
//   resolve_one   one primary's pixel from its S radiances
// Nothing here calls a libm transcendental function: raygen_common.hpp's device cosf / sinf are why
// AO directions agree with the host only to a few ulp, and a path must not drift from its host
// statement bounce after bounce. Both sides are built with -ffp-contract=off; the device file
// without denormal flushing and with correctly rounded division and square root (Makefile), so
// every float is the IEEE value on both sides. Only the bits of a NaN that an operation makes
// differ (x86 0xFFC00000, gfx950 0x7FC00000).
#pragma once
#include <cmath>
#include <cstdint>

#include "light_common.hpp"

namespace mrt {
namespace path {

constexpr uint32_t kGolden = 0x9e3779b9u;

// A path between two vertices: 16 bytes. task < 0: the slot holds no path (in-place mode).
struct State {
    float tr, tg, tb;   // throughput
    int32_t task;       // the path's index in its batch: input ray * S + sample
};

// What does not change over a call.
struct Params {
    int32_t vertex, depth, numSamples;
    uint32_t seed;
    float lightPos[3], lightRadius, lightColor[3], sky[3], maxDist;
    const float* triNormals;
    const uint32_t* triMaterialColor;
    int64_t numTris;
};

// What one slot's vertex step gives.
struct Step {
    bool survivor;      // the path hit: shadow, pending, bounce and state are to be written
    bool escaped;       // the path left the scene at a vertex >= 1: add[] goes to its radiance
    float add[3];
    int32_t task;
    State state;
    float pending[3];
    rg::RayRec shadow, bounce;
};

// A slot's task names a path of the batch: a radiance entry to add to.
MRT_HD inline bool owns(int32_t task, int32_t numPaths) { return (uint32_t)task < (uint32_t)numPaths; }
MRT_HD inline State first_state(int32_t slot) { return State{1.0f, 1.0f, 1.0f, slot}; }
MRT_HD inline State dead_state() { return State{0.0f, 0.0f, 0.0f, -1}; }
MRT_HD inline rg::RayRec dead_ray() { return rg::RayRec{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f}; }

MRT_HD inline void hash_words(uint32_t seed, int32_t vertex, uint32_t key, float offset[3], float shift[2]) {
    uint32_t a = seed + (uint32_t)vertex * kGolden + key, b = kGolden, c = kGolden;
    rg::jenkins_mix(a, b, c);
    rg::jenkins_mix(a, b, c);
    offset[0] = (float)a * 0x1p-32f;
    offset[1] = (float)b * 0x1p-32f;
    offset[2] = (float)c * 0x1p-32f;
    rg::jenkins_mix(a, b, c);
    shift[0] = (float)a * 0x1p-32f;
    shift[1] = (float)b * 0x1p-32f;
}

MRT_HD inline void halton23(int s, float h[2]) {
    float x = 0.0f, xadd = 1.0f;
    for (unsigned hc2 = (unsigned)s + 1; hc2 != 0; hc2 >>= 1) {
        xadd *= 0.5f;
        if (hc2 & 1) x += xadd;
    }
    float y = 0.0f, yadd = 1.0f;
    for (int hc3 = s + 1; hc3 != 0; hc3 /= 3) {
        yadd *= 1.0f / 3.0f;
        y += (float)(hc3 % 3) * yadd;
    }
    h[0] = x;
    h[1] = y;
}

// (pi/2)^k / k! with alternating signs, rounded to float32.
constexpr float kSin1 = 1.5707963267948966f, kSin3 = -0.6459640975062462f, kSin5 = 0.07969262624616703f,
                kSin7 = -0.004681754135318687f, kSin9 = 0.00016044118478735975f;
constexpr float kCos2 = -1.2337005501361697f, kCos4 = 0.253669507901048f, kCos6 = -0.020863480763352957f,
                kCos8 = 0.0009192602748394263f, kCos10 = -2.5202042373060596e-05f;

MRT_HD inline void sincos_turn(float u, float* cosOut, float* sinOut) {
    const float v = u * 4.0f;
    int q = (int)v;
    float f = v - (float)q;
    if (f > 0.5f) {
        f = f - 1.0f;
        q = q + 1;
    }
    const float f2 = f * f;
    const float s = f * (kSin1 + f2 * (kSin3 + f2 * (kSin5 + f2 * (kSin7 + f2 * kSin9))));
    const float c = 1.0f + f2 * (kCos2 + f2 * (kCos4 + f2 * (kCos6 + f2 * (kCos8 + f2 * kCos10))));
    switch (q & 3) {
        case 0: *cosOut = c; *sinOut = s; break;
        case 1: *cosOut = -s; *sinOut = c; break;
        case 2: *cosOut = -c; *sinOut = -s; break;
        default: *cosOut = s; *sinOut = -c; break;
    }
}

MRT_HD inline float wrap1(float p) {
    if (p >= 1.0f) p -= 1.0f;
    return p;
}

MRT_HD inline rg::V3 bounce_dir(rg::V3 nf, int s, const float shift[2]) {
    float h[2];
    halton23(s, h);
    const float u1 = wrap1(h[0] + shift[0]), u2 = wrap1(h[1] + shift[1]);
    float cs, sn;
    sincos_turn(u2, &cs, &sn);
    const float r = sqrtf(u1);
    const float x = r * cs, y = r * sn;
    const float z = sqrtf(rg::fw_max(1.0f - x * x - y * y, 0.0f));
    const rg::V3 na = rg::vabs(nf);
    const float nm = rg::fw_max(rg::fw_max(na.x, na.y), na.z);
    rg::V3 perp = rg::make(nf.y, -nf.x, 0.0f);
    if (nm == na.z) perp = rg::make(0.0f, nf.z, -nf.y);
    else if (nm == na.x) perp = rg::make(-nf.z, 0.0f, nf.x);
    perp = rg::normalize(perp);
    const rg::V3 biperp = rg::cross(nf, perp);
    return rg::normalize(rg::add(rg::add(rg::scale(perp, x), rg::scale(biperp, y)), rg::scale(nf, z)));
}

// The vertex step of one live path: `in` its current ray, (id, t) that ray's result, st its state
// (first_state(slot) at vertex 0). An id outside [0, numTris) is a miss.
MRT_HD inline void extend(const Params& p, const rg::RayRec& in, int32_t id, float t, const State& st, Step& out) {
    out.task = st.task;
    out.survivor = false;
    out.escaped = false;
    if (!(id >= 0 && (int64_t)id < p.numTris)) {
        if (p.vertex >= 1) {
            out.escaped = true;
            out.add[0] = st.tr * p.sky[0];
            out.add[1] = st.tg * p.sky[1];
            out.add[2] = st.tb * p.sky[2];
        }
        return;
    }
    out.survivor = true;
    const int S = p.numSamples;
    const int32_t input = st.task / S;
    const int s = st.task - input * S;
    float origin[3], offset[3], shift[2], albedo[4];
    light::shadow_origin(in, t, origin);
    const float* n = p.triNormals + 3 * (int64_t)id;
    const rg::V3 d = rg::make(in.dx, in.dy, in.dz);
    rg::V3 nf = rg::make(n[0], n[1], n[2]);
    if (rg::dot(nf, d) > 0.0f) nf = rg::neg(nf);
    light::from_abgr(p.triMaterialColor[id], albedo);
    out.state = State{st.tr * albedo[0], st.tg * albedo[1], st.tb * albedo[2], st.task};
    hash_words(p.seed, p.vertex, p.vertex == 0 ? (uint32_t)input : (uint32_t)st.task, offset, shift);
    out.shadow = light::shadow_ray(origin, offset, id, s, S, p.lightPos, p.lightRadius);
    const float k = light::lit_factor(in, t, n, p.lightPos);
    out.pending[0] = out.state.tr * p.lightColor[0] * k;
    out.pending[1] = out.state.tg * p.lightColor[1] * k;
    out.pending[2] = out.state.tb * p.lightColor[2] * k;
    if (p.vertex < p.depth) {
        const rg::V3 dir = bounce_dir(nf, s, shift);
        out.bounce = rg::RayRec{origin[0], origin[1], origin[2], 0.0f, dir.x, dir.y, dir.z, p.maxDist};
    } else {
        out.bounce = dead_ray();
    }
}

// One primary's value from its S paths' radiances (4 floats each, the fourth unused): the sum from
// 0 in sample order times 1 / S.
MRT_HD inline void resolve_one(const float* radiance, int S, float value[4]) {
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int s = 0; s < S; s++)
        for (int c = 0; c < 3; c++) sum[c] += radiance[4 * (int64_t)s + c];
    const float inv = 1.0f / (float)S;
    value[0] = sum[0] * inv;
    value[1] = sum[1] * inv;
    value[2] = sum[2] * inv;
    value[3] = 1.0f;
}

MRT_HD inline void background(float value[4]) {
    value[0] = 0.2f;
    value[1] = 0.4f;
    value[2] = 0.8f;
    value[3] = 1.0f;
}

}  // namespace path
}  // namespace mrt
