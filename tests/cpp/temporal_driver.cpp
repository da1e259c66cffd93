// temporal_driver.cpp — the host statements of the temporal accumulation (csrc/host/temporal.cpp:
// mrth_temporal_motion, mrth_temporal_accumulate) and its plan (csrc/temporal_plan.cpp) as a
// stand-alone program: tests/test_temporal.py runs the Makefile's copy for the plan and builds a
// second copy with -fsanitize=address,undefined. Host compiler only, no HIP. Every buffer is a
// vector of exactly the size the call may touch, so a stray access is the sanitizer's to report.
//
//   temporal_driver motion <numPixels> <slotToId> <rays> <results> <triangles> <vertices> <prevVertices> <outPrevPosition>
//       prevPosition starts as zeros
//   temporal_driver accumulate <scalars> <image> <guide> <albedo> <prevPosition | -> <prevGuide | -> <prevHistory | ->
//                              <outHistory> <outImage | -> <outPixels | ->
//       scalars: 24 words: width height havePrev maxHistory normalCos sigmaPlane (floats as bits),
//       the 16 words of prevWorldToScreen, the 2 of prevSubpixel
//   temporal_driver plan <width> <height> <maxHistory> <normalCos bits> <sigmaPlane bits> <variant>
//       prints rc tiled grid tilesX tilesY and the bits of invPlane
//   temporal_driver plan-motion <numPrimary> <numTris> <numVertices> <numPixels>     prints rc empty grid
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gpu-ray-tracing_amd/csrc/temporal_plan.hpp"
#include "mrt_host.h"

namespace {

template <class T>
std::vector<T> read_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

template <class T>
void write_file(const std::string& path, const std::vector<T>& v) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) std::exit(2);
    std::fclose(f);
}

int failed(const char* what, int rc) {
    std::fprintf(stderr, "%s: %d (%s)\n", what, rc, mrth_last_error());
    return 1;
}

float as_float(uint32_t w) {
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}

uint32_t as_bits(float f) {
    uint32_t w;
    std::memcpy(&w, &f, 4);
    return w;
}

bool given(const char* arg) { return std::strcmp(arg, "-") != 0; }

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "motion" && argc == 10) {
        const int32_t numPixels = (int32_t)std::atol(argv[2]);
        const std::vector<int32_t> s2i = read_file<int32_t>(argv[3]);
        const std::vector<float> rays = read_file<float>(argv[4]);
        const std::vector<int32_t> results = read_file<int32_t>(argv[5]);
        const std::vector<int32_t> triangles = read_file<int32_t>(argv[6]);
        const std::vector<float> vertices = read_file<float>(argv[7]);
        const std::vector<float> prevVertices = read_file<float>(argv[8]);
        if (rays.size() != 8 * s2i.size() || results.size() != 4 * s2i.size() || vertices.size() != prevVertices.size()) return 2;
        std::vector<float> prevPosition(4 * (size_t)numPixels);
        const int rc = mrth_temporal_motion((int32_t)s2i.size(), s2i.data(), rays.data(), results.data(), triangles.data(),
                                            (int64_t)(triangles.size() / 3), vertices.data(), prevVertices.data(),
                                            (int64_t)(vertices.size() / 3), numPixels, prevPosition.data());
        if (rc != MRTH_OK) return failed("mrth_temporal_motion", rc);
        write_file(argv[9], prevPosition);
        return 0;
    }
    if (mode == "accumulate" && argc == 12) {
        const std::vector<uint32_t> w = read_file<uint32_t>(argv[2]);
        if (w.size() != 24) return 2;
        const std::vector<float> image = read_file<float>(argv[3]);
        const std::vector<float> guide = read_file<float>(argv[4]);
        const std::vector<float> albedo = read_file<float>(argv[5]);
        const std::vector<float> prevPosition = given(argv[6]) ? read_file<float>(argv[6]) : std::vector<float>();
        const std::vector<float> prevGuide = given(argv[7]) ? read_file<float>(argv[7]) : std::vector<float>();
        const std::vector<float> prevHistory = given(argv[8]) ? read_file<float>(argv[8]) : std::vector<float>();
        const bool wantImage = given(argv[10]), wantPixels = given(argv[11]);
        mrth_temporal_params p{};
        p.width = (int32_t)w[0];
        p.height = (int32_t)w[1];
        p.havePrev = (int32_t)w[2];
        p.maxHistory = (int32_t)w[3];
        p.normalCos = as_float(w[4]);
        p.sigmaPlane = as_float(w[5]);
        for (int i = 0; i < 16; i++) p.prevWorldToScreen[i] = as_float(w[6 + i]);
        p.prevSubpixel[0] = as_float(w[22]);
        p.prevSubpixel[1] = as_float(w[23]);
        const size_t px = (size_t)p.width * (size_t)p.height;
        if (image.size() != 4 * px || guide.size() != 8 * px || albedo.size() != 4 * px) return 2;
        if ((given(argv[6]) && prevPosition.size() != 4 * px) || (given(argv[7]) && prevGuide.size() != 8 * px) ||
            (given(argv[8]) && prevHistory.size() != 4 * px))
            return 2;
        std::vector<float> history(4 * px), out(wantImage ? 4 * px : 0);
        std::vector<uint32_t> pixels(wantPixels ? px : 0);
        p.image = image.data();
        p.guide = guide.data();
        p.albedo = albedo.data();
        p.prevPosition = given(argv[6]) ? prevPosition.data() : nullptr;
        p.prevGuide = given(argv[7]) ? prevGuide.data() : nullptr;
        p.prevHistory = given(argv[8]) ? prevHistory.data() : nullptr;
        p.history = history.data();
        p.imageOut = wantImage ? out.data() : nullptr;
        p.pixels = wantPixels ? pixels.data() : nullptr;
        const int rc = mrth_temporal_accumulate(&p);
        if (rc != MRTH_OK) return failed("mrth_temporal_accumulate", rc);
        write_file(argv[9], history);
        if (wantImage) write_file(argv[10], out);
        if (wantPixels) write_file(argv[11], pixels);
        return 0;
    }
    if (mode == "plan" && argc == 8) {
        const mrt::TemporalPlan p = mrt::plan_temporal_accumulate(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                                                  as_float((uint32_t)std::strtoul(argv[5], nullptr, 0)),
                                                                  as_float((uint32_t)std::strtoul(argv[6], nullptr, 0)),
                                                                  std::atoi(argv[7]));
        std::printf("%d %d %d %d %d %u\n", p.rc, p.tiled, p.grid, p.tilesX, p.tilesY, as_bits(p.invPlane));
        return 0;
    }
    if (mode == "plan-motion" && argc == 6) {
        const mrt::TemporalPlan p =
            mrt::plan_temporal_motion((int32_t)std::atol(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), (int32_t)std::atol(argv[5]));
        std::printf("%d %d %d\n", p.rc, p.empty ? 1 : 0, p.grid);
        return 0;
    }
    std::fprintf(stderr, "usage: temporal_driver motion|accumulate|plan|plan-motion ... (see the head of tests/cpp/temporal_driver.cpp)\n");
    return 2;
}
