// wide_plan_driver — the device derivation's level scheme (csrc/wide_kernel.hip, sequenced by
// csrc/derive_api.cpp) run sequentially on the CPU through the same per-node steps
// (csrc/wide_common.hpp): host compiler, no HIP. tests/test_wide_plan.py compares what it writes
// with mrt_refit_plan and mrt_derive_wide_nodes, and feeds it trees that are none.
//
//   wide_plan_driver <nodes.bin> <woop.bin | -> <out.bin> [reverse]
//
// nodes.bin: Compact2 records (64 bytes each); woop.bin: the Woop array (16 bytes per slot; "-":
// none, the leaf refs carry no counts). reverse: every level is walked from its last node to its
// first (a level's nodes are independent, so the result must not change). Prints one line:
//   ok levels=<height levels> depth=<depth levels> wide=<wide nodes> bound=<stack bound>
//   refused <refit_levels' reason>
// and on "ok" writes int32 {levels, wide, bound, n}, order[n], offsets[levels + 1],
// wide[32 * wide], src[4 * wide].
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gpu-ray-tracing_amd/csrc/wide_common.hpp"

namespace w = mrt::wide;

static bool read_file(const char* path, std::vector<int32_t>* out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out->resize((size_t)bytes / 4);
    const bool ok = std::fread(out->data(), 4, out->size(), f) == out->size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: wide_plan_driver nodes.bin woop.bin|- out.bin [reverse]\n");
        return 2;
    }
    const bool reverse = argc > 4 && std::string(argv[4]) == "reverse";
    std::vector<int32_t> nodes, woop;
    if (!read_file(argv[1], &nodes) || nodes.empty() || nodes.size() % 16) {
        std::fprintf(stderr, "bad node file\n");
        return 2;
    }
    const bool haveWoop = std::string(argv[2]) != "-";
    if (haveWoop && (!read_file(argv[2], &woop) || woop.size() % 4)) {
        std::fprintf(stderr, "bad woop file\n");
        return 2;
    }
    const int32_t n = (int32_t)(nodes.size() / 16);
    const size_t N = (size_t)n;
    std::vector<int32_t> visited(N, 0), byDepth(N, 0), height(N, 0), size(N, 0), kids(4 * N, 0), index(N, 0),
        entries(N, 0), summary(w::kSummaryWords, 0);
    w::Derive d{};
    d.nodes = nodes.data();
    d.numNodes = n;
    const int64_t slots = (int64_t)woop.size() / 4;
    d.woopX = haveWoop && slots <= ((int64_t)1 << w::kLeafAddrBits) ? woop.data() : nullptr;
    d.woopStride = 4;
    d.woopSlots = slots;
    d.visited = visited.data();
    d.byDepth = byDepth.data();
    d.height = height.data();
    d.size = size.data();
    d.kids = kids.data();
    d.index = index.data();
    d.entries = entries.data();
    d.summary = summary.data();
    visited[0] = 1;
    size[0] = 1;
    summary[w::kReached] = 1;

    // One level's nodes through a step, in either order.
    auto walk = [&](int begin, int end, void (*step)(const w::Derive&, int32_t)) {
        for (int k = 0; k < end - begin; k++) step(d, byDepth[(size_t)(reverse ? end - 1 - k : begin + k)]);
    };
    // The counters the kernels keep once per wave: the nodes reached, the stack bound.
    auto expand = +[](const w::Derive& dd, int32_t node) {
        int32_t kid[2];
        const int cnt = w::step_claim(dd, node, kid);
        for (int k = 0; k < cnt; k++) {
            const int32_t pos = dd.summary[w::kReached]++;
            if (pos < dd.numNodes) dd.byDepth[pos] = kid[k];
        }
    };
    auto number = +[](const w::Derive& dd, int32_t node) {
        dd.summary[w::kStackBound] = std::max(dd.summary[w::kStackBound], w::step_index(dd, node));
    };

    // Topology: level by level; a level claims at least one new node or the walk ends, so at
    // most n levels.
    std::vector<int32_t> depth{0};
    for (int begin = 0, end = 1; begin < end;) {
        if ((int64_t)depth.size() > (int64_t)n + 1) {
            std::printf("refused the topology pass did not end\n");
            return 1;
        }
        walk(begin, end, expand);
        begin = end;
        end = std::min(summary[w::kReached], n);
        depth.push_back(begin);
    }
    if (const char* why = w::error_text(summary[w::kError], summary[w::kReached], n)) {
        std::printf("refused %s\n", why);
        return 0;
    }
    const int levels = (int)depth.size() - 1;
    for (int l = levels - 1; l >= 0; l--) walk(depth[(size_t)l], depth[(size_t)l + 1], w::step_height);
    const int top = height[0];   // node 0's height is the tree's
    std::vector<int32_t> order(N);
    for (int32_t i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return height[(size_t)a] < height[(size_t)b]; });
    // the level starts are where the sorted height changes; every height 0 .. top occurs
    std::vector<int32_t> offsets((size_t)top + 2, -1);
    offsets[(size_t)top + 1] = n;
    for (int32_t i = 0; i < n; i++) {
        const int32_t h = height[(size_t)order[(size_t)i]];
        if (h >= 0 && h <= top && (i == 0 || height[(size_t)order[(size_t)i - 1]] != h)) offsets[(size_t)h] = i;
    }

    // Collapse: roots down, sizes up, numbers down, then every node's emission.
    for (int l = 0; l < levels; l++) walk(depth[(size_t)l], depth[(size_t)l + 1], w::step_flag);
    for (int l = levels - 1; l >= 0; l--) walk(depth[(size_t)l], depth[(size_t)l + 1], w::step_size);
    const int32_t numWide = size[0];
    if (summary[w::kError] || numWide < 1 || numWide > n) {
        std::printf("refused the collapse left the tree\n");
        return 1;
    }
    for (int l = 0; l < levels; l++) walk(depth[(size_t)l], depth[(size_t)l + 1], number);
    std::vector<uint32_t> wide((size_t)numWide * 32, 0xdeadbeefu);
    std::vector<int32_t> src((size_t)numWide * 4, -7);
    d.numWide = numWide;
    for (int32_t k = 0; k < n; k++) {
        const int32_t node = reverse ? n - 1 - k : k;
        uint32_t o[32];
        int32_t s4[4], at = 0;
        if (!w::step_emit(d, node, o, s4, &at)) continue;
        std::memcpy(wide.data() + (size_t)at * 32, o, sizeof(o));
        std::memcpy(src.data() + (size_t)at * 4, s4, sizeof(s4));
    }

    FILE* f = std::fopen(argv[3], "wb");
    if (!f) {
        std::fprintf(stderr, "cannot write %s\n", argv[3]);
        return 2;
    }
    const int32_t head[4] = {top + 1, numWide, summary[w::kStackBound], n};
    std::fwrite(head, 4, 4, f);
    std::fwrite(order.data(), 4, order.size(), f);
    std::fwrite(offsets.data(), 4, offsets.size(), f);
    std::fwrite(wide.data(), 4, wide.size(), f);
    std::fwrite(src.data(), 4, src.size(), f);
    std::fclose(f);
    std::printf("ok levels=%d depth=%d wide=%d bound=%d\n", top + 1, levels, numWide, summary[w::kStackBound]);
    return 0;
}
