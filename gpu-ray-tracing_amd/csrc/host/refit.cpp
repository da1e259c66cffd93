// refit.cpp — refit of Compact2 buffers in place for moved vertices (the CPU
// reference of the device refit, csrc/refit_kernel.hip, and mrth_bvh_refit).
//
// The tree's topology, triIndex and the terminators stay; what depends on vertex
// positions is recomputed with the serialiser's arithmetic (woop_common.hpp):
// a leaf is walked from its first Woop slot in steps of three up to the slot whose
// x bits are the terminator's (only Z rows are looked at: a U or V row may hold
// -0.0 too), inner boxes are unions of the child record's two boxes, children
// before parents.
#include <cstring>
#include <string>
#include <vector>

#include "bvh.hpp"

namespace mrt {

namespace {

woop::Box load_box(const int32_t* rec, int child) {
    woop::Box b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = bits_float((uint32_t)rec[woop::box_word(child, k)]);
        b.hi[k] = bits_float((uint32_t)rec[woop::box_word(child, k) + 1]);
    }
    return b;
}

void store_box(int32_t* rec, int child, const woop::Box& b) {
    for (int k = 0; k < 3; k++) {
        rec[woop::box_word(child, k)] = (int32_t)float_bits(b.lo[k]);
        rec[woop::box_word(child, k) + 1] = (int32_t)float_bits(b.hi[k]);
    }
}

}  // namespace

bool refit_compact2(Compact2& c, const float* vertices, int64_t numVertices, const int32_t* triangles,
                    int64_t numTriangles, std::string* err) {
    auto fail = [&](const char* what) {
        if (err) *err = what;
        return false;
    };
    const int64_t numNodes = (int64_t)c.nodes.size() / 16;
    const int64_t slots = (int64_t)c.woop.size() / 4;
    if (numNodes < 1 || (int64_t)c.triIndex.size() != slots) return fail("refit: buffers are not Compact2-shaped");
    if (numVertices < 0 || numTriangles < 0 || (numVertices && !vertices) || (numTriangles && !triangles))
        return fail("refit: bad vertex / triangle arrays");

    // Pass 1 (writes nothing): the nodes parent before child, and every reference checked.
    std::vector<int64_t> order;
    order.reserve((size_t)numNodes);
    std::vector<char> seen((size_t)numNodes, 0);
    std::vector<int64_t> stack{0};
    seen[0] = 1;
    while (!stack.empty()) {
        const int64_t n = stack.back();
        stack.pop_back();
        order.push_back(n);
        for (int i = 0; i < 2; i++) {
            const int32_t ref = c.nodes[(size_t)n * 16 + 12 + i];
            if (ref >= 0) {
                const int64_t child = ref / 4;
                if (ref % 4 || child >= numNodes || seen[(size_t)child]) return fail("refit: the nodes are not a tree");
                seen[(size_t)child] = 1;
                stack.push_back(child);
                continue;
            }
            int64_t s = ~(int64_t)ref;
            for (;; s += 3) {
                if (s >= slots) return fail("refit: a leaf runs past the Woop array");
                if ((uint32_t)c.woop[(size_t)s * 4] == woop::kTerminatorBits) break;
                if (s + 2 >= slots) return fail("refit: a leaf runs past the Woop array");
                const int32_t tri = c.triIndex[(size_t)s];
                if (tri < 0 || tri >= numTriangles) return fail("refit: triIndex entry out of range");
                for (int k = 0; k < 3; k++) {
                    const int32_t v = triangles[(size_t)tri * 3 + k];
                    if (v < 0 || v >= numVertices) return fail("refit: vertex index out of range");
                }
            }
        }
    }

    // Pass 2: children before parents. valid[2n + i]: child i of node n holds a triangle
    // somewhere below it (an empty leaf keeps its box and is left out of every union).
    std::vector<char> valid((size_t)numNodes * 2, 0);
    for (size_t o = order.size(); o-- > 0;) {
        const int64_t n = order[o];
        int32_t* rec = &c.nodes[(size_t)n * 16];
        for (int i = 0; i < 2; i++) {
            const int32_t ref = rec[12 + i];
            if (ref >= 0) {
                const int64_t child = ref / 4;
                const int32_t* crec = &c.nodes[(size_t)child * 16];
                const bool v0 = valid[(size_t)child * 2] != 0, v1 = valid[(size_t)child * 2 + 1] != 0;
                if (!v0 && !v1) continue;
                const woop::Box b0 = load_box(crec, 0), b1 = load_box(crec, 1);
                store_box(rec, i, v0 && v1 ? woop::box_union(b0, b1) : (v0 ? b0 : b1));
                valid[(size_t)n * 2 + i] = 1;
                continue;
            }
            woop::Box box = woop::box_empty();
            bool any = false;
            for (int64_t s = ~(int64_t)ref; (uint32_t)c.woop[(size_t)s * 4] != woop::kTerminatorBits; s += 3) {
                const int32_t* t = &triangles[(size_t)c.triIndex[(size_t)s] * 3];
                const float* v[3] = {vertices + (size_t)t[0] * 3, vertices + (size_t)t[1] * 3, vertices + (size_t)t[2] * 3};
                float rows[12];
                woop::woop_rows(v[0], v[1], v[2], rows);
                woop::woop_guard(rows);
                std::memcpy(&c.woop[(size_t)s * 4], rows, sizeof rows);
                for (int k = 0; k < 3; k++) woop::box_grow(box, v[k]);
                any = true;
            }
            if (!any) continue;
            store_box(rec, i, box);
            valid[(size_t)n * 2 + i] = 1;
        }
    }
    return true;
}

}  // namespace mrt
