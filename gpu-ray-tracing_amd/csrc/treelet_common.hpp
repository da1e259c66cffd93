// treelet_common.hpp — the restructuring of one treelet of a Compact2 tree (Karras & Aila
// 2013), computed identically on the host (csrc/host/treelet.cpp, g++) and on the device
// (csrc/treelet_kernel.hip, hipcc), so that both write the same bytes (the role
// lbvh_common.hpp has for the build and woop_common.hpp for the refit):
//   form         the treelet below a root record: its two child slots, then the inner leaf of
//                largest area replaced by its two children (a tie: the earliest in the list; the
//                children go to the end of the list) until there are kMaxLeaves leaves or no inner
//                one. The records absorbed this way are the treelet's internal records.
//   area         float32 dx*dy + dy*dz + dz*dx, left to right
//   leaves_ok    no leaf box with lo > hi on an axis
//   subset_area  a[S]: the area of the union of the leaf boxes of S, folded in ascending leaf order
//   solve_subset c[S] = a[S] + min over proper partitions (c[P] + c[S \ P]), c[{i}] = 0, the
//                root's own a left out; P holds the lowest set bit of S, and of equal sums the
//                lowest P wins. Needs every smaller subset solved: any order by subset size.
//   emit         the root keeps its record; the internal records are reused in the order they
//                were absorbed, handed out breadth first (child 0 before child 1). A slot gets its
//                subset's ref and box: a treelet leaf's are moved as they are, an inner subset's
//                box is the union (woop::box_union, child 0's then child 1's) of the two boxes
//                its own record gets, so the refit's invariant holds by construction.
//   restructure  all of it for one root, sequentially: the statement both sides must equal.
// A treelet is left bit for bit when it has fewer than 3 leaves, when a leaf box is inverted,
// when any a[S] is not finite, when the optimum is not strictly below the sum of the internal
// records' areas (added in the order they were absorbed), or when the union of the root's two
// new boxes would not be, bit for bit, the union of its two old ones: min / max keep the later
// of -0.0 and +0.0, so another order of uniting can flip the sign of a zero plane, and boxes that
// are not the unions of what lies below them (a clipped SBVH's) can differ outright; the slot
// above the root is moved or left, never recomputed. Words 14-15, Woop rows, triIndex and
// terminators are never touched. Both sides are built with -ffp-contract=off, the device file
// without denormal flushing (Makefile): every float here is the IEEE value.
#pragma once
#include <cstdint>

#include "woop_common.hpp"

namespace mrt {
namespace treelet {

constexpr int kMaxLeaves = 7;
constexpr int kSubsets = 1 << kMaxLeaves;
constexpr int kMaxInternal = kMaxLeaves - 2;   // besides the root

struct Treelet {
    int n;                          // leaves
    int32_t ref[kMaxLeaves];        // the slot's word 12 / 13, moved as it is
    woop::Box box[kMaxLeaves];
    int32_t internal[kMaxInternal]; // n - 2 absorbed records, in order
    float original;                 // the sum of their areas
    woop::Box whole;                // the union of the root's two boxes as they were
};

struct Dp {
    float a[kSubsets];
    float c[kSubsets];
    uint8_t part[kSubsets];         // the chosen P of S (0: a single leaf)
};

MRT_HD inline float bits_to_float(uint32_t u) {
    union {
        uint32_t u;
        float f;
    } x;
    x.u = u;
    return x.f;
}
MRT_HD inline uint32_t float_to_bits(float f) {
    union {
        uint32_t u;
        float f;
    } x;
    x.f = f;
    return x.u;
}

MRT_HD inline woop::Box load_box(const uint32_t* rec, int child) {
    woop::Box b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = bits_to_float(rec[woop::box_word(child, k)]);
        b.hi[k] = bits_to_float(rec[woop::box_word(child, k) + 1]);
    }
    return b;
}
MRT_HD inline void store_box(uint32_t* rec, int child, const woop::Box& b) {
    for (int k = 0; k < 3; k++) {
        rec[woop::box_word(child, k)] = float_to_bits(b.lo[k]);
        rec[woop::box_word(child, k) + 1] = float_to_bits(b.hi[k]);
    }
}

MRT_HD inline float area(const woop::Box& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}

// +-inf and NaN have every exponent bit set.
MRT_HD inline bool finite(float f) { return (float_to_bits(f) & 0x7f800000u) != 0x7f800000u; }

// A ref that may be followed: an inner child inside the node array, not the root itself.
MRT_HD inline bool inner_ref(int32_t ref, int64_t numNodes, int64_t root) {
    return ref >= 0 && (ref & 3) == 0 && (ref >> 2) < numNodes && (ref >> 2) != root;
}

MRT_HD inline void form(const uint32_t* nodes, int64_t numNodes, int64_t root, Treelet& t) {
    const uint32_t* rec = nodes + root * 16;
    t.n = 2;
    for (int i = 0; i < 2; i++) {
        t.ref[i] = (int32_t)rec[12 + i];
        t.box[i] = load_box(rec, i);
    }
    t.whole = woop::box_union(t.box[0], t.box[1]);
    t.original = 0.0f;
    int absorbed = 0;
    while (t.n < kMaxLeaves) {
        int best = -1;
        float bestArea = 0.0f;
        for (int i = 0; i < t.n; i++) {
            if (!inner_ref(t.ref[i], numNodes, root)) continue;
            bool again = false;   // a malformed array only: a record is absorbed once
            for (int k = 0; k < absorbed; k++) again |= t.internal[k] == (t.ref[i] >> 2);
            if (again) continue;
            const float ar = area(t.box[i]);
            if (best < 0 || ar > bestArea) {
                best = i;
                bestArea = ar;
            }
        }
        if (best < 0) break;
        const int32_t child = t.ref[best] >> 2;
        t.internal[absorbed++] = child;
        t.original += bestArea;
        for (int i = best; i + 1 < t.n; i++) {
            t.ref[i] = t.ref[i + 1];
            t.box[i] = t.box[i + 1];
        }
        const uint32_t* crec = nodes + (int64_t)child * 16;
        for (int i = 0; i < 2; i++) {
            t.ref[t.n - 1 + i] = (int32_t)crec[12 + i];
            t.box[t.n - 1 + i] = load_box(crec, i);
        }
        t.n++;
    }
}

MRT_HD inline bool leaves_ok(const Treelet& t) {
    if (t.n < 3) return false;
    for (int i = 0; i < t.n; i++)
        for (int k = 0; k < 3; k++)
            if (t.box[i].lo[k] > t.box[i].hi[k]) return false;
    return true;
}

// S != 0, below 1 << t.n.
MRT_HD inline float subset_area(const Treelet& t, int S) {
    woop::Box b{};
    bool first = true;
    for (int i = 0; i < t.n; i++) {
        if (!(S >> i & 1)) continue;
        b = first ? t.box[i] : woop::box_union(b, t.box[i]);
        first = false;
    }
    return area(b);
}

// d.a filled, every proper subset of S solved.
MRT_HD inline void solve_subset(Dp& d, int S, int full) {
    const int low = S & -S, rest = S ^ low;
    if (!rest) {
        d.c[S] = 0.0f;
        d.part[S] = 0;
        return;
    }
    int bestP = low;
    float best = d.c[low] + d.c[rest];
    for (int sub = (0 - rest) & rest; sub != rest; sub = (sub - rest) & rest) {   // ascending, proper
        const int P = low | sub;
        const float cost = d.c[P] + d.c[S ^ P];
        if (cost < best) {
            best = cost;
            bestP = P;
        }
    }
    d.c[S] = S == full ? best : d.a[S] + best;
    d.part[S] = (uint8_t)bestP;
}

MRT_HD inline bool worth_it(const Treelet& t, const Dp& d) { return d.c[(1 << t.n) - 1] < t.original; }

MRT_HD inline bool same_bits(const woop::Box& a, const woop::Box& b) {
    for (int k = 0; k < 3; k++)
        if (float_to_bits(a.lo[k]) != float_to_bits(b.lo[k]) || float_to_bits(a.hi[k]) != float_to_bits(b.hi[k]))
            return false;
    return true;
}

// The n - 1 records of the optimum written over the root's and the internal records' slots.
// False, and nothing written, where the union of the root's two new boxes would not be the
// bits of the union of its two old ones (t.whole): the slot above the root is not this
// treelet's to write, and it must stay the union of the root's boxes where it was.
MRT_HD inline bool emit(uint32_t* nodes, int64_t root, const Treelet& t, const Dp& d) {
    int64_t record[kMaxLeaves - 1];
    int subset[kMaxLeaves - 1];
    int childRec[kMaxLeaves - 1][2];   // the queue entry of an inner child, -1: a treelet leaf
    record[0] = root;
    subset[0] = (1 << t.n) - 1;
    int count = 1;
    for (int q = 0; q < count; q++) {
        const int P = d.part[subset[q]];
        const int side[2] = {P, subset[q] ^ P};
        for (int i = 0; i < 2; i++) {
            if (!(side[i] & (side[i] - 1))) {
                childRec[q][i] = -1;
                continue;
            }
            record[count] = t.internal[count - 1];
            subset[count] = side[i];
            childRec[q][i] = count++;
        }
    }
    // Last handed out first: an inner child's two boxes are final before its parent unites them.
    woop::Box box[kMaxLeaves - 1][2], whole[kMaxLeaves - 1];
    uint32_t ref[kMaxLeaves - 1][2];
    for (int q = count - 1; q >= 0; q--) {
        const int P = d.part[subset[q]];
        const int side[2] = {P, subset[q] ^ P};
        for (int i = 0; i < 2; i++) {
            if (childRec[q][i] < 0) {
                int leaf = 0;
                while (!(side[i] >> leaf & 1)) leaf++;
                box[q][i] = t.box[leaf];
                ref[q][i] = (uint32_t)t.ref[leaf];
            } else {
                box[q][i] = whole[childRec[q][i]];
                ref[q][i] = (uint32_t)(record[childRec[q][i]] * 4);
            }
        }
        whole[q] = woop::box_union(box[q][0], box[q][1]);
    }
    if (!same_bits(whole[0], t.whole)) return false;
    for (int q = 0; q < count; q++) {
        uint32_t* rec = nodes + record[q] * 16;
        for (int i = 0; i < 2; i++) {
            store_box(rec, i, box[q][i]);
            rec[12 + i] = ref[q][i];
        }
    }
    return true;
}

// The whole step for one root, sequentially. True: the treelet was rewritten.
MRT_HD inline bool restructure(uint32_t* nodes, int64_t numNodes, int64_t root) {
    Treelet t;
    form(nodes, numNodes, root, t);
    if (!leaves_ok(t)) return false;
    Dp d;
    const int full = (1 << t.n) - 1;
    for (int S = 1; S <= full; S++) {
        d.a[S] = subset_area(t, S);
        if (!finite(d.a[S])) return false;
    }
    for (int S = 1; S <= full; S++) solve_subset(d, S, full);   // a proper subset of S is below S
    return worth_it(t, d) && emit(nodes, root, t, d);
}

}  // namespace treelet
}  // namespace mrt
