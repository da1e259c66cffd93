// denoise_driver.cpp — the host statements of the denoiser (csrc/host/denoise.cpp:
// mrth_denoise_features, mrth_denoise_filter) and its plan (csrc/denoise_plan.cpp) as a stand-alone
// program: tests/test_denoise.py runs the Makefile's copy for the plan and builds a second copy
// with -fsanitize=address,undefined. Host compiler only, no HIP. Every buffer is a vector of
// exactly the size the call may touch, so a stray access is the sanitizer's to report.
//
//   denoise_driver features <numPixels> <slotToId> <rays> <results> <normals> <material> <outGuide> <outAlbedo>
//       guide and albedo start as zeros
//   denoise_driver filter <scalars> <image> <guide> <albedo> <outImage | -> <outPixels | ->
//       scalars: 6 words: width height iterations normalSquarings sigmaColor sigmaPlane (floats as bits)
//   denoise_driver plan <width> <height> <iterations> <squarings> <sigmaColor bits> <sigmaPlane bits> <variant>
//       prints rc launches and the bits of invPlane, then per step a line: step tiled grid tilesX
//       tilesY residues ldsBytes and the bits of invColor2
//   denoise_driver plan-features <numPrimary> <numTris> <numPixels>     prints rc empty grid
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gpu-ray-tracing_amd/csrc/denoise_plan.hpp"
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

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "features" && argc == 10) {
        const int32_t numPixels = (int32_t)std::atol(argv[2]);
        const std::vector<int32_t> s2i = read_file<int32_t>(argv[3]);
        const std::vector<float> rays = read_file<float>(argv[4]);
        const std::vector<int32_t> results = read_file<int32_t>(argv[5]);
        const std::vector<float> normals = read_file<float>(argv[6]);
        const std::vector<uint32_t> material = read_file<uint32_t>(argv[7]);
        if (rays.size() != 8 * s2i.size() || results.size() != 4 * s2i.size() || normals.size() != 3 * material.size()) return 2;
        std::vector<float> guide(8 * (size_t)numPixels), albedo(4 * (size_t)numPixels);
        const int rc = mrth_denoise_features((int32_t)s2i.size(), s2i.data(), rays.data(), results.data(), normals.data(),
                                             material.data(), (int64_t)material.size(), numPixels, guide.data(), albedo.data());
        if (rc != MRTH_OK) return failed("mrth_denoise_features", rc);
        write_file(argv[8], guide);
        write_file(argv[9], albedo);
        return 0;
    }
    if (mode == "filter" && argc == 8) {
        const std::vector<uint32_t> w = read_file<uint32_t>(argv[2]);
        if (w.size() != 6) return 2;
        const std::vector<float> image = read_file<float>(argv[3]);
        const std::vector<float> guide = read_file<float>(argv[4]);
        const std::vector<float> albedo = read_file<float>(argv[5]);
        const bool wantImage = std::strcmp(argv[6], "-") != 0, wantPixels = std::strcmp(argv[7], "-") != 0;
        mrth_denoise_params p{};
        p.width = (int32_t)w[0];
        p.height = (int32_t)w[1];
        p.iterations = (int32_t)w[2];
        p.normalSquarings = (int32_t)w[3];
        p.sigmaColor = as_float(w[4]);
        p.sigmaPlane = as_float(w[5]);
        const size_t px = (size_t)p.width * (size_t)p.height;
        if (image.size() != 4 * px || guide.size() != 8 * px || albedo.size() != 4 * px) return 2;
        std::vector<float> s0(p.iterations >= 2 ? 4 * px : 0), s1(p.iterations >= 3 ? 4 * px : 0), out(wantImage ? 4 * px : 0);
        std::vector<uint32_t> pixels(wantPixels ? px : 0);
        p.image = image.data();
        p.guide = guide.data();
        p.albedo = albedo.data();
        p.scratch[0] = s0.empty() ? nullptr : s0.data();
        p.scratch[1] = s1.empty() ? nullptr : s1.data();
        p.imageOut = wantImage ? out.data() : nullptr;
        p.pixels = wantPixels ? pixels.data() : nullptr;
        const int rc = mrth_denoise_filter(&p);
        if (rc != MRTH_OK) return failed("mrth_denoise_filter", rc);
        if (wantImage) write_file(argv[6], out);
        if (wantPixels) write_file(argv[7], pixels);
        return 0;
    }
    if (mode == "plan" && argc == 9) {
        const mrt::DenoisePlan p = mrt::plan_denoise_filter(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                                                            as_float((uint32_t)std::strtoul(argv[6], nullptr, 0)),
                                                            as_float((uint32_t)std::strtoul(argv[7], nullptr, 0)), std::atoi(argv[8]));
        std::printf("%d %d %u\n", p.rc, p.launches, as_bits(p.invPlane));
        for (int k = 0; k < mrt::denoise::kMaxIterations && p.rc == 0; k++) {
            const mrt::DenoiseLaunchPlan& it = p.at[k];
            std::printf("%d %d %d %d %d %d %d %u\n", it.step, it.tiled, it.grid, it.tilesX, it.tilesY, it.residues, it.ldsBytes,
                        as_bits(it.invColor2));
        }
        return 0;
    }
    if (mode == "plan-features" && argc == 5) {
        const mrt::DenoisePlan p = mrt::plan_denoise_features((int32_t)std::atol(argv[2]), std::atoll(argv[3]), (int32_t)std::atol(argv[4]));
        std::printf("%d %d %d\n", p.rc, p.empty ? 1 : 0, p.grid);
        return 0;
    }
    std::fprintf(stderr, "usage: denoise_driver features|filter|plan|plan-features ... (see the head of tests/cpp/denoise_driver.cpp)\n");
    return 2;
}
