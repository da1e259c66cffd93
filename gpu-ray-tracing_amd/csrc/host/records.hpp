// records.hpp — the reference's 16-byte RayResult and how the host statements read and write the
// records of a caller's untyped buffers. It depends on nothing but the two standard headers: the
// stand-alone test programs build path.cpp, denoise.cpp and temporal.cpp without scene.hpp.
#pragma once
#include <cstdint>
#include <cstring>

namespace mrt {

// reference src/rt/Util.hh:79-89 — 16 B; the trace writes {id, t} only.
struct RayResult {
    int32_t id;
    float t;
    int32_t padA;
    int32_t padB;
};
static_assert(sizeof(RayResult) == 16, "RayResult must be 16 bytes");

// Record `at` of an array of T behind an untyped pointer of any alignment.
template <class T>
T get_record(const void* base, int64_t at) {
    T v;
    std::memcpy(&v, static_cast<const char*>(base) + (int64_t)sizeof(T) * at, sizeof(T));
    return v;
}

template <class T>
void put_record(void* base, int64_t at, const T& v) {
    std::memcpy(static_cast<char*>(base) + (int64_t)sizeof(T) * at, &v, sizeof(T));
}

}  // namespace mrt
