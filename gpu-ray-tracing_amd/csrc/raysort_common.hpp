// raysort_common.hpp — everything a Morton sort of a ray batch must compute identically on the
// host (csrc/host/raysort.cpp, g++) and on the device (csrc/raysort_kernel.hip, hipcc), so that
// both give the same keys, permutation, rays and id maps (the role lbvh_common.hpp has for the
// device build). The key is the reference's (RayBuffer::mortonSort, RayBuffer.cc:256-324,
// genMortonKeysKernel, RayBufferKernels.cu:146-180) with its sequence of operations taken in IEEE
// arithmetic: the reference compiles it under fast-math, so its own bits are not defined.
//   box_grow      the min / max over the rays' origins (and end points), independent of the order
//   components    a = (o - lo) / (hi - lo), b = (d / |d| + 1) / 2, per axis
//   convert       float -> fixed point, every non-finite and out-of-range case spelled out
//   ray_key       the six components' bits interleaved: bit 6 i + c of the key is bit i of
//                 component c, c = 0..5 = q_x, q_y, q_z, r_x, r_y, r_z (collectBits)
//   shifted_word  64 bits of key >> 6 * drop_levels: what one pass of the LSD sort orders by
// Both sides are built with -ffp-contract=off; the device file without denormal flushing and with
// correctly rounded division and square root (Makefile).
#pragma once
#include <cmath>
#include <cstdint>

#include "woop_common.hpp"

namespace mrt {
namespace raysort {

constexpr int kMaxDropLevels = 24;       // drop_levels 0..24
constexpr int kKeyWords = 6;             // hash[0..5], hash[5] most significant
constexpr int kKeyLevels = 25;           // bit levels a component can hold: q <= 2^24
constexpr uint32_t kOriginCap = 16777216u;      // 2^24
constexpr uint32_t kDirectionCap = 2097152u;    // 2^21
constexpr int64_t kMaxRays = (int64_t)1 << 30;

// lo / hi of the rays' points as (lo.xyz, hi.xyz); the reference's start values. A NaN never
// enters (the comparisons are false), and only the sign of a zero depends on the order of growing
// and merging: o - lo and hi - lo give the same float for either zero except where the result is
// itself a zero or a NaN, and both convert to 0. So any order gives the same keys.
struct Box {
    float lo[3], hi[3];
};
MRT_HD inline Box box_empty() {
    const float big = 3.402823466e+38f;   // FLT_MAX
    return Box{{big, big, big}, {-big, -big, -big}};
}
MRT_HD inline void box_grow(Box& b, const float p[3]) {
    for (int k = 0; k < 3; k++) {
        if (p[k] < b.lo[k]) b.lo[k] = p[k];
        if (p[k] > b.hi[k]) b.hi[k] = p[k];
    }
}
// lo against lo and hi against hi only: an empty o changes nothing.
MRT_HD inline void box_merge(Box& b, const Box& o) {
    for (int k = 0; k < 3; k++) {
        if (o.lo[k] < b.lo[k]) b.lo[k] = o.lo[k];
        if (o.hi[k] > b.hi[k]) b.hi[k] = o.hi[k];
    }
}

// A ray's contribution: its origin and, in box mode 0 (the reference's, RayBufferKernels.cu:94-102),
// its end point o + d * tmax: one multiply, one add. ray = (o.xyz, tmin, d.xyz, tmax).
MRT_HD inline void box_grow_ray(Box& b, const float ray[8], int boxMode) {
    const float o[3] = {ray[0], ray[1], ray[2]};
    box_grow(b, o);
    if (boxMode == 0) {
        float e[3];
        for (int k = 0; k < 3; k++) {
            const float step = ray[4 + k] * ray[7];
            e[k] = o[k] + step;
        }
        box_grow(b, e);
    }
}

// NaN -> 0, x <= 0 -> 0, x >= cap -> cap, else truncation.
MRT_HD inline uint32_t convert(float x, uint32_t cap) {
    if (!(x > 0.0f)) return 0;
    if (x >= (float)cap) return cap;
    return (uint32_t)x;
}

// The six components of a ray's key, in key order.
MRT_HD inline void components(const float ray[8], const Box& box, uint32_t comp[6]) {
    const float dx = ray[4], dy = ray[5], dz = ray[6];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float sum = (xx + yy) + zz;
    const float len = sqrtf(sum);
    for (int k = 0; k < 3; k++) {
        const float ext = box.hi[k] - box.lo[k];
        const float a = (ray[k] - box.lo[k]) / ext;
        const float b = (ray[4 + k] / len + 1.0f) * 0.5f;
        const float qa = a * 256.0f;
        const float qb = b * 32.0f;
        comp[k] = convert(qa * 65536.0f, kOriginCap);
        comp[3 + k] = convert(qb * 65536.0f, kDirectionCap);
    }
}

// hash[w] = key bits 32 w .. 32 w + 31. With the caps hash[5] is 0 and hash[4] below 2^22.
MRT_HD inline void interleave(const uint32_t comp[6], uint32_t hash[kKeyWords]) {
    uint64_t w[3] = {0, 0, 0};
MRT_UNROLL
    for (int i = 0; i < kKeyLevels; i++) {
        uint64_t g = 0;
MRT_UNROLL
        for (int c = 0; c < 6; c++) g |= (uint64_t)((comp[c] >> i) & 1u) << c;
        const int at = 6 * i, word = at >> 6, sh = at & 63;
        w[word] |= g << sh;
        if (sh > 58) w[word + 1] |= g >> (64 - sh);   // at most bit 149: word + 1 <= 2
    }
    for (int k = 0; k < 3; k++) {
        hash[2 * k] = (uint32_t)w[k];
        hash[2 * k + 1] = (uint32_t)(w[k] >> 32);
    }
}

MRT_HD inline void ray_key(const float ray[8], const Box& box, uint32_t hash[kKeyWords]) {
    uint32_t comp[6];
    components(ray, box, comp);
    interleave(comp, hash);
}

// The order is ascending by key >> 6 * dropLevels, ties by ascending input slot: an LSD sort over
// the 64-bit words of the shifted key, least significant first, each pass stable.
MRT_HD inline int shifted_bits(int dropLevels) { return 6 * (kKeyLevels - dropLevels); }   // 150 .. 6
MRT_HD inline int sort_passes(int dropLevels) { return (shifted_bits(dropLevels) + 63) / 64; }
// Bits of pass `pass` that can be set: the sort's end_bit (begin_bit is 0).
MRT_HD inline int pass_bits(int dropLevels, int pass) {
    const int left = shifted_bits(dropLevels) - 64 * pass;
    return left < 64 ? left : 64;
}
// Bits [64 pass, 64 pass + 64) of key >> 6 * dropLevels.
MRT_HD inline uint64_t shifted_word(const uint32_t hash[kKeyWords], int dropLevels, int pass) {
    const int at = 6 * dropLevels + 64 * pass, i = at >> 5, sh = at & 31;
    const uint64_t h0 = i < kKeyWords ? hash[i] : 0u, h1 = i + 1 < kKeyWords ? hash[i + 1] : 0u,
                   h2 = i + 2 < kKeyWords ? hash[i + 2] : 0u;
    const uint64_t v = h0 | h1 << 32;
    return sh ? v >> sh | h2 << (64 - sh) : v;
}

}  // namespace raysort
}  // namespace mrt
