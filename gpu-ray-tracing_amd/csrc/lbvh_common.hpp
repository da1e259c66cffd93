// lbvh_common.hpp — everything a linear BVH build must compute identically on the
// host (csrc/host/lbvh.cpp, g++) and on the device (csrc/lbvh_kernel.hip, hipcc), so
// that both emit the same Compact2 bytes (the role woop_common.hpp has for the refit):
//   tri_centroid   the middle of a triangle's box
//   bounds_grow    the min / max over all centroids, independent of the order
//   quantize       21 bits per axis, one float32 rounding per operation
//   morton63       x, y, z interleaved, x the most significant bit of each triple
//   delta          the common-prefix length of two sorted positions (Karras 2012,
//                  equal codes continued by the positions' own bits)
//   karras_node    range and split of internal node i by binary search on delta
// Both sides are built with -ffp-contract=off; the device file without denormal
// flushing and with correctly rounded division (Makefile).
#pragma once
#include <cstdint>

#include "woop_common.hpp"

namespace mrt {
namespace lbvh {

constexpr int kMaxLeafLimit = 8;         // max_leaf_size 1..8
// The refit's limits (refit_kernel.hpp) on what a build may emit: 4N + 1 slots < 2^28.
constexpr int64_t kMaxTriangles = (((int64_t)1 << 28) - 2) / 4;

// Upper bounds of what a build of n triangles writes: n - 1 records (at least one),
// 3n + leaves <= 4n slots, and the one-record tree's second terminator.
MRT_HD inline int64_t max_records(int64_t n) { return n > 2 ? n - 1 : 1; }
MRT_HD inline int64_t max_slots(int64_t n) { return 4 * n + 1; }

MRT_HD inline bool tri_in_range(const int32_t* t, int64_t numVertices) {
    const uint64_t nv = (uint64_t)numVertices;
    return (uint64_t)(int64_t)t[0] < nv && (uint64_t)(int64_t)t[1] < nv && (uint64_t)(int64_t)t[2] < nv;
}

// c = (bmin + bmax) * 0.5f per axis, bmin / bmax over the three vertices.
MRT_HD inline void tri_centroid(const float* v0, const float* v1, const float* v2, float c[3]) {
    for (int k = 0; k < 3; k++) {
        const float lo = woop::fw_min(woop::fw_min(v0[k], v1[k]), v2[k]);
        const float hi = woop::fw_max(woop::fw_max(v0[k], v1[k]), v2[k]);
        c[k] = (lo + hi) * 0.5f;
    }
}

// lo / hi of all centroids as (lo.xyz, hi.xyz). A NaN never enters and the sign of a
// zero never shows in a key, so any order of growing and merging gives the same keys.
struct Bounds {
    float lo[3], hi[3];
};
MRT_HD inline Bounds bounds_empty() {
    const float inf = __builtin_huge_valf();
    return Bounds{{inf, inf, inf}, {-inf, -inf, -inf}};
}
MRT_HD inline void bounds_grow(Bounds& b, const float c[3]) {
    for (int k = 0; k < 3; k++) {
        if (c[k] < b.lo[k]) b.lo[k] = c[k];
        if (c[k] > b.hi[k]) b.hi[k] = c[k];
    }
}
// lo against lo and hi against hi only: an empty o (+inf, -inf) changes nothing.
MRT_HD inline void bounds_merge(Bounds& b, const Bounds& o) {
    for (int k = 0; k < 3; k++) {
        if (o.lo[k] < b.lo[k]) b.lo[k] = o.lo[k];
        if (o.hi[k] > b.hi[k]) b.hi[k] = o.hi[k];
    }
}

// q = ext > 0 ? min(2097151, (uint32)((c - lo) / ext * 2097152.0f)) : 0, a NaN to 0.
MRT_HD inline uint32_t quantize(float c, float lo, float ext) {
    if (!(ext > 0.0f)) return 0;
    const float f = (c - lo) / ext * 2097152.0f;
    if (!(f >= 0.0f)) return 0;
    return f >= 2097151.0f ? 2097151u : (uint32_t)f;
}

// Bit i of v to bit 3i.
MRT_HD inline uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x001f00000000ffffull;
    x = (x | x << 16) & 0x001f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
MRT_HD inline uint64_t morton63(uint32_t qx, uint32_t qy, uint32_t qz) {
    return spread3(qx) << 2 | spread3(qy) << 1 | spread3(qz);
}

// The key of a triangle whose vertex indices are in range.
MRT_HD inline uint64_t tri_code(const float c[3], const Bounds& b) {
    uint32_t q[3];
    for (int k = 0; k < 3; k++) q[k] = quantize(c[k], b.lo[k], b.hi[k] - b.lo[k]);
    return morton63(q[0], q[1], q[2]);
}

// Common-prefix length of sorted positions i and j (i in range, i != j); -1 outside.
MRT_HD inline int delta(const uint64_t* codes, int n, int i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = codes[i] ^ codes[j];
    if (x) return __builtin_clzll(x);
    return 64 + __builtin_clz((uint32_t)i ^ (uint32_t)j);
}

// Internal node i of the Karras hierarchy over n >= 2 sorted keys: it covers sorted
// positions [first, last]; its children cover [first, split] and [split + 1, last]. A
// child range of more than one position is internal node split (left) or split + 1 (right).
struct Node {
    int first, last, split;
};
MRT_HD inline Node karras_node(const uint64_t* codes, int n, int i) {
    const int64_t d = delta(codes, n, i, (int64_t)i + 1) > delta(codes, n, i, (int64_t)i - 1) ? 1 : -1;
    const int dmin = delta(codes, n, i, i - d);
    int64_t lmax = 2;
    while (delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = delta(codes, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t split = i + s * d + (d < 0 ? -1 : 0);
    return Node{(int)(d > 0 ? i : j), (int)(d > 0 ? j : i), (int)split};
}

// Numbering: the leaf of rank r that starts at sorted position p has its
// first Woop slot at 3p + r and its terminator at 3(last + 1) + r.
MRT_HD inline int leaf_slot(int p, int rank) { return 3 * p + rank; }

}  // namespace lbvh
}  // namespace mrt
