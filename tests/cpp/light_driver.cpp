// light_driver.cpp — the host statements of the area light (csrc/host/light.cpp: mrth_shadow_rays,
// mrth_reconstruct_lit) as a stand-alone program, so that tests/test_light.py can run them under
// -fsanitize=address,undefined with nothing preloaded. Every array is exactly as long as the call
// may touch, so a read or write past an end is a report.
//
//   light_driver shadow <rays> <results> <numInput> <numSamples> <light: 3 floats + radius> <seed> <out>
//   light_driver lit <n> <first> <count> <slotToId> <rays> <results> <batchIdToSlot | -> <batchResults>
//                    <normals> <material> <light: 3 floats> <numPixels> <out>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
void write_file(const char* path, const std::vector<T>& v) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f || (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) std::exit(2);
    std::fclose(f);
}

int failed(const char* what, int rc) {
    std::fprintf(stderr, "%s: %d (%s)\n", what, rc, mrth_last_error());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "shadow" && argc == 9) {
        const std::vector<float> rays = read_file<float>(argv[2]);
        const std::vector<int32_t> results = read_file<int32_t>(argv[3]);
        const long n = std::atol(argv[4]), samples = std::atol(argv[5]);
        const std::vector<float> light = read_file<float>(argv[6]);
        const uint32_t seed = (uint32_t)std::strtoul(argv[7], nullptr, 0);
        if ((long)rays.size() != 8 * n || (long)results.size() != 4 * n || light.size() != 4) return 2;
        std::vector<float> out((size_t)(8 * n * samples));
        const int rc = mrth_shadow_rays(rays.data(), results.data(), n, (int32_t)samples, light.data(), light[3], seed,
                                        out.data());
        if (rc) return failed("mrth_shadow_rays", rc);
        write_file(argv[8], out);
        return 0;
    }
    if (mode == "lit" && argc == 15) {
        const int n = std::atoi(argv[2]), first = std::atoi(argv[3]), count = std::atoi(argv[4]);
        const std::vector<int32_t> s2i = read_file<int32_t>(argv[5]);
        const std::vector<float> rays = read_file<float>(argv[6]);
        const std::vector<int32_t> results = read_file<int32_t>(argv[7]);
        const bool identity = std::strcmp(argv[8], "-") == 0;
        const std::vector<int32_t> b2s = identity ? std::vector<int32_t>() : read_file<int32_t>(argv[8]);
        const std::vector<int32_t> batch = read_file<int32_t>(argv[9]);
        const std::vector<float> normals = read_file<float>(argv[10]);
        const std::vector<uint32_t> material = read_file<uint32_t>(argv[11]);
        const std::vector<float> light = read_file<float>(argv[12]);
        if (light.size() != 3 || (long)batch.size() != 4L * n * count) return 2;
        std::vector<uint32_t> pixels((size_t)std::atol(argv[13]), 0u);
        const int rc = mrth_reconstruct_lit(n, first, count, s2i.data(), rays.data(), results.data(),
                                            identity ? nullptr : b2s.data(), batch.data(), normals.data(), material.data(),
                                            light.data(), pixels.data());
        if (rc) return failed("mrth_reconstruct_lit", rc);
        write_file(argv[14], pixels);
        return 0;
    }
    std::fprintf(stderr, "usage: light_driver shadow|lit ... (see the head of tests/cpp/light_driver.cpp)\n");
    return 2;
}
