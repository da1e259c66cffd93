// wide_common.hpp — the arithmetic of the exact 4-wide derivation and of the refit plan, shared
// verbatim by the host derivation (csrc/wide_bvh.cpp, g++ or hipcc's host pass), the gfx950
// kernels that derive both on the device (csrc/wide_kernel.hip) and the sequential CPU driver of
// the level scheme (tests/cpp/wide_plan_driver.cpp), so all three choose the same children and
// write the same bytes:
//   Child, binary_children   a Compact2 record's two children (ref, box bits, source slot)
//   half_area                double: x * y + y * z + z * x
//   collapse                 the children of the wide node rooted at a binary node: the inner
//                            child of largest area is replaced by its two children until there
//                            are four (strict >: the first index wins a tie, a NaN area is never
//                            picked)
//   wide_leaf_ref            a leaf ref with its triangle count
//   wide_node_words          the 32 words of one exact wide node (layout: wide_bvh.cpp)
// and the per-node steps of the level scheme: every step reads only what an earlier
// level wrote, so the kernels run them one launch per level and the driver one loop per level.
// Both sides are built with -ffp-contract=off (a contracted fma in the area would pick other
// children); the device file is built without denormal flushing (a flushed float would convert
// to another double).
#pragma once
#include <cstdint>

#ifndef MRT_HD
#if defined(__HIPCC__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif

namespace mrt {
namespace wide {

constexpr int32_t kSentinel = 0x76543210;   // an absent child's ref (kEntrypointSentinel)
constexpr int kLeafAddrBits = 27;           // kWideLeafAddrBits
constexpr uint32_t kQuietNaN = 0x7fc00000u; // an absent child's planes
constexpr int32_t kTerminator = (int32_t)0x80000000;

struct Child {
    int32_t ref;
    float lo[3], hi[3];
    int32_t src;   // the Compact2 slot the box was read from: binary node * 2 + side
};

MRT_HD inline float as_float(int32_t i) {
    float f;
    __builtin_memcpy(&f, &i, 4);
    return f;
}

MRT_HD inline uint32_t as_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// An inner ref that addresses a record of the array: the first float4 of a record below numNodes.
MRT_HD inline bool inner_ref(int32_t ref, int64_t numNodes) {
    return ref >= 0 && ref != kSentinel && (ref & 3) == 0 && (ref >> 2) < numNodes;
}

MRT_HD inline void binary_children(const int32_t* nodes, int32_t ref, Child out[2]) {
    const int32_t* n = nodes + (int64_t)(ref / 4) * 16;
    const int32_t src = (ref / 4) * 2;
    out[0] = Child{n[12], {as_float(n[0]), as_float(n[2]), as_float(n[8])}, {as_float(n[1]), as_float(n[3]), as_float(n[9])}, src};
    out[1] = Child{n[13], {as_float(n[4]), as_float(n[6]), as_float(n[10])}, {as_float(n[5]), as_float(n[7]), as_float(n[11])},
                   src + 1};
}

MRT_HD inline double half_area(const Child& c) {
    const double x = (double)c.hi[0] - c.lo[0], y = (double)c.hi[1] - c.lo[1], z = (double)c.hi[2] - c.lo[2];
    return x * y + y * z + z * x;
}

// The children of the wide node rooted at binary node `ref` (an inner_ref). A child whose ref
// is not a record of the array is never opened (*bad is set: not a tree).
MRT_HD inline int collapse(const int32_t* nodes, int64_t numNodes, int32_t ref, Child out[4], bool* bad) {
    Child two[2];
    binary_children(nodes, ref, two);
    out[0] = two[0];
    out[1] = two[1];
    int n = 2;
    while (n < 4) {
        int best = -1;
        double bestArea = -1.0;
        for (int i = 0; i < n; i++) {
            if (out[i].ref < 0) continue;
            if (!inner_ref(out[i].ref, numNodes)) {
                *bad = true;
                continue;
            }
            if (half_area(out[i]) > bestArea) {
                bestArea = half_area(out[i]);
                best = i;
            }
        }
        if (best < 0) break;
        binary_children(nodes, out[best].ref, two);
        for (int i = n; i > best + 1; i--) out[i] = out[i - 1];   // the two grandchildren take best's place
        out[best] = two[0];
        out[best + 1] = two[1];
        n++;
    }
    return n;
}

// The ref a wide child stores for Compact2 leaf ref `ref`: with the first word of every Woop
// slot (woopX at `stride` words per slot; null: no counts) it carries the triangle count.
MRT_HD inline int32_t wide_leaf_ref(int32_t ref, const int32_t* woopX, int64_t stride, int64_t woopSlots) {
    if (!woopX) return ref;
    const int64_t slot = ~(int64_t)ref;
    int32_t count = 0;
    for (int32_t k = 0; k <= 15; k++) {
        const int64_t s = slot + 3 * (int64_t)k;
        if (s >= woopSlots) break;
        if (woopX[s * stride] == kTerminator) {
            count = k;
            break;
        }
    }
    return ~(int32_t)(slot | ((int64_t)count << kLeafAddrBits));
}

// One exact wide node: the planes of children [0, n), NaN planes and the sentinel for the
// absent ones, refs[c] for the present ones, words 28-31 zero; src4 (may be null) gets the
// source slots, -1 for an absent child.
MRT_HD inline void wide_node_words(const Child ch[4], int n, const int32_t refs[4], uint32_t o[32], int32_t* src4) {
    for (int c = 0; c < 4; c++) {
        const int f4 = c >> 1, pair = (c & 1) * 2;   // children 0,1 in float4 0/2/4, 2,3 in 1/3/5
        for (int k = 0; k < 3; k++) {
            o[(2 * k + f4) * 4 + pair] = c < n ? as_bits(ch[c].lo[k]) : kQuietNaN;
            o[(2 * k + f4) * 4 + pair + 1] = c < n ? as_bits(ch[c].hi[k]) : kQuietNaN;
        }
        o[24 + c] = (uint32_t)(c < n ? refs[c] : kSentinel);
        o[28 + c] = 0u;
        if (src4) src4[c] = c < n ? ch[c].src : -1;
    }
}

// ---- the level scheme --------------------------------------------------------------------
// On the device the claims and the error bits are atomics; the sequential driver runs plain ones.
// The counters (nodes reached, the stack bound) are the caller's: the kernels add to them once
// per wave, the driver directly.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline int32_t fetch_set(int32_t* p) { return atomicExch(p, 1); }
__device__ inline void fetch_or(int32_t* p, int32_t v) { atomicOr(p, v); }
#else
inline int32_t fetch_set(int32_t* p) {
    const int32_t old = *p;
    *p = 1;
    return old;
}
inline void fetch_or(int32_t* p, int32_t v) { *p |= v; }
#endif

// The summary words (the fixed-size readback).
// kNextLevel / kFrontBegin / kFrontEnd: where a chained topology launch stopped.
enum : int { kReached = 0, kError = 1, kStackBound = 3, kNextLevel = 4, kFrontBegin = 5, kFrontEnd = 6,
             kSummaryWords = 8 };
enum : int32_t { kErrRef = 1, kErrTwice = 2 };

// What refit_levels (refit_plan.cpp) says of the same defects.
inline const char* error_text(int32_t error, int64_t reached, int64_t numNodes) {
    if (error & kErrRef) return "a child ref points outside the node array";
    if (error & kErrTwice) return "a node record is reached twice (not a tree)";
    if (reached != numNodes) return "a node record is not reachable from node 0";
    return nullptr;
}

// One derivation's buffers; n = numNodes. Zeroed before the first step: visited, size, summary;
// then visited[0] = 1, byDepth[0] = 0, summary[kReached] = 1, size[0] = 1 (node 0 is
// reached and is a wide root), index[0] = entries[0] = 0.
struct Derive {
    const int32_t* nodes;   // n Compact2 records
    int32_t numNodes;
    const int32_t* woopX;   // first words of the Woop slots at woopStride words per slot (null: no counts)
    int32_t woopStride;
    int64_t woopSlots;
    int32_t* visited;       // n: claimed by the topology pass
    int32_t* byDepth;       // n: the nodes breadth first, depth level by depth level
    int32_t* height;        // n
    int32_t* size;          // n: 0 = not a wide root, else the wide nodes of its wide subtree
    int32_t* kids;          // 4n: a wide root's child refs (Compact2 refs; kSentinel = absent)
    int32_t* index;         // n: a wide root's depth-first number
    int32_t* entries;       // n: stack entries when a wide root is visited
    int32_t* summary;       // kSummaryWords
    uint32_t* wideOut;      // 32 words per wide node
    int32_t* srcOut;        // 4 per wide node
    int32_t numWide;
};

// Topology, going down: claims node n's inner children; returns how many it claimed (0..2,
// in kid[]). The caller appends them to byDepth and counts them in summary[kReached].
MRT_HD inline int step_claim(const Derive& d, int32_t n, int32_t kid[2]) {
    int count = 0;
    if ((uint32_t)n >= (uint32_t)d.numNodes) return 0;
    for (int side = 0; side < 2; side++) {
        const int32_t ref = d.nodes[(int64_t)n * 16 + 12 + side];
        if (ref < 0) continue;   // a leaf
        if (!inner_ref(ref, d.numNodes)) {
            fetch_or(d.summary + kError, kErrRef);
            continue;
        }
        if (fetch_set(d.visited + (ref >> 2))) {   // claimed before: a DAG or a cycle ends here
            fetch_or(d.summary + kError, kErrTwice);
            continue;
        }
        kid[count++] = ref >> 2;
    }
    return count;
}

// Heights, going up: 0 for two leaf children, else 1 + the highest inner child. Node 0's is the
// tree's.
MRT_HD inline void step_height(const Derive& d, int32_t n) {
    if ((uint32_t)n >= (uint32_t)d.numNodes) return;
    int32_t h = 0;
    for (int side = 0; side < 2; side++) {
        const int32_t ref = d.nodes[(int64_t)n * 16 + 12 + side];
        if (inner_ref(ref, d.numNodes) && d.height[ref >> 2] + 1 > h) h = d.height[ref >> 2] + 1;
    }
    d.height[n] = h;
}

// Collapse, going down: a wide root keeps its children's refs and flags the inner ones as roots.
MRT_HD inline void step_flag(const Derive& d, int32_t n) {
    if ((uint32_t)n >= (uint32_t)d.numNodes || d.size[n] == 0) return;
    Child ch[4];
    bool bad = false;
    const int cnt = collapse(d.nodes, d.numNodes, n * 4, ch, &bad);
    for (int i = 0; i < 4; i++) {
        const int32_t ref = i < cnt ? ch[i].ref : kSentinel;
        d.kids[(int64_t)n * 4 + i] = ref;
        if (ref < 0 || ref == kSentinel) continue;
        if (inner_ref(ref, d.numNodes)) d.size[ref >> 2] = 1;
        else bad = true;
    }
    if (bad) fetch_or(d.summary + kError, kErrRef);
}

// Sizes, going up: 1 + the sizes of the inner wide children.
MRT_HD inline void step_size(const Derive& d, int32_t n) {
    if ((uint32_t)n >= (uint32_t)d.numNodes || d.size[n] == 0) return;
    int32_t s = 1;
    for (int i = 0; i < 4; i++) {
        const int32_t ref = d.kids[(int64_t)n * 4 + i];
        if (inner_ref(ref, d.numNodes)) s += d.size[ref >> 2];
    }
    d.size[n] = s;
}

// Depth-first numbers and stack entries, going down (number_wide's and wide_stack_bound's).
// Returns the entries below wide root n (0 for other nodes): their maximum is the stack bound.
MRT_HD inline int32_t step_index(const Derive& d, int32_t n) {
    if ((uint32_t)n >= (uint32_t)d.numNodes || d.size[n] == 0) return 0;
    int present = 0;
    for (int i = 0; i < 4; i++) present += d.kids[(int64_t)n * 4 + i] != kSentinel;
    const int32_t below = d.entries[n] + (present > 1 ? present - 1 : 0);   // pushes all but the child it enters
    int32_t next = d.index[n] + 1;
    for (int i = 0; i < 4; i++) {
        const int32_t ref = d.kids[(int64_t)n * 4 + i];
        if (!inner_ref(ref, d.numNodes)) continue;
        d.index[ref >> 2] = next;
        d.entries[ref >> 2] = below;
        next += d.size[ref >> 2];
    }
    return below;
}

// Emission, any order: wide root n's node into `o` and its source slots into src4; false when
// n is no wide root or its number lies outside the array.
MRT_HD inline bool step_emit(const Derive& d, int32_t n, uint32_t o[32], int32_t src4[4], int32_t* at) {
    if ((uint32_t)n >= (uint32_t)d.numNodes || d.size[n] == 0) return false;
    const int32_t w = d.index[n];
    if ((uint32_t)w >= (uint32_t)d.numWide) return false;
    Child ch[4];
    bool bad = false;
    const int cnt = collapse(d.nodes, d.numNodes, n * 4, ch, &bad);
    int32_t refs[4] = {kSentinel, kSentinel, kSentinel, kSentinel};
    for (int c = 0; c < cnt; c++) {
        if (ch[c].ref < 0) refs[c] = wide_leaf_ref(ch[c].ref, d.woopX, d.woopStride, d.woopSlots);
        else if (inner_ref(ch[c].ref, d.numNodes)) refs[c] = d.index[ch[c].ref >> 2] * 8;
    }
    wide_node_words(ch, cnt, refs, o, src4);
    *at = w;
    return true;
}

}  // namespace wide
}  // namespace mrt
