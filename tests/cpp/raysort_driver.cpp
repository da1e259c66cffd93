// raysort_driver.cpp — mrth_ray_sort (csrc/host/raysort.cpp) as a stand-alone program, for
// tests/test_raysort.py to build with -fsanitize=address,undefined and run on its edge batches:
//   raysort_driver rays.bin numRays dropLevels box out.bin [ids.bin]
// rays.bin: numRays * 8 float32; ids.bin: numRays int32 (absent: NULL, the identity). out.bin:
// rays (32 n bytes), id_to_slot (4 n, started at -1), slot_to_id (4 n), keys (24 n), box (24).
// Every buffer is a heap allocation of exactly its size, so a write past one is reported.
// The layouts of mrt.h's reference-compatible sort structs are checked here at compile time.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mrt.h"
#include "mrt_host.h"

static_assert(sizeof(mrt_morton_key) == 28 && offsetof(mrt_morton_key, hash) == 4, "MortonKey");
static_assert(sizeof(mrt_find_aabb_input) == 16 && offsetof(mrt_find_aabb_input, inRays) == 8, "FindAABBInput");
static_assert(sizeof(mrt_find_aabb_output) == 24 && offsetof(mrt_find_aabb_output, aabbHi) == 12, "FindAABBOutput");
static_assert(sizeof(mrt_gen_morton_keys_input) == 48 && offsetof(mrt_gen_morton_keys_input, inRays) == 32 &&
                  offsetof(mrt_gen_morton_keys_input, outKeys) == 40,
              "GenMortonKeysInput");
static_assert(sizeof(mrt_reorder_rays_input) == 56 && offsetof(mrt_reorder_rays_input, inKeys) == 8 &&
                  offsetof(mrt_reorder_rays_input, outSlotToID) == 48,
              "ReorderRaysInput");
static_assert(sizeof(mrt_ray_sort_params) == 8 && sizeof(mrth_ray_sort_params) == 8, "ray sort params");

template <class T>
static bool read_all(const char* path, std::vector<T>& out, size_t count) {
    out.resize(count);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = count ? std::fread(out.data(), sizeof(T), count, f) : 0;
    std::fclose(f);
    return got == count;
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s rays.bin numRays dropLevels box out.bin [ids.bin]\n", argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[2]);
    const mrth_ray_sort_params params{std::atoi(argv[3]), std::atoi(argv[4])};
    const size_t N = n > 0 ? (size_t)n : 0;
    std::vector<float> rays;
    std::vector<int32_t> ids;
    if (!read_all(argv[1], rays, N * 8) || (argc > 6 && !read_all(argv[6], ids, N))) {
        std::fprintf(stderr, "cannot read the input\n");
        return 2;
    }
    std::vector<float> outRays(N * 8), box(6);
    std::vector<int32_t> idToSlot(N, -1), slotToId(N);
    std::vector<uint32_t> keys(N * 6);
    const int rc = mrth_ray_sort(rays.data(), argc > 6 ? ids.data() : nullptr, n, &params, outRays.data(), idToSlot.data(),
                                 slotToId.data(), keys.data(), box.data());
    if (rc != MRTH_OK) {
        std::fprintf(stderr, "mrth_ray_sort: %d (%s)\n", rc, mrth_last_error());
        return 1;
    }
    // once more with every optional output absent
    std::vector<float> again(N * 8);
    if (mrth_ray_sort(rays.data(), nullptr, n, nullptr, again.data(), nullptr, nullptr, nullptr, nullptr) != MRTH_OK) return 1;
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    auto put = [f](const void* p, size_t words) {
        if (words) std::fwrite(p, 4, words, f);
    };
    put(outRays.data(), outRays.size());
    put(idToSlot.data(), idToSlot.size());
    put(slotToId.data(), slotToId.size());
    put(keys.data(), keys.size());
    put(box.data(), box.size());
    std::fclose(f);
    std::printf("sorted %d rays\n", n);
    return 0;
}
