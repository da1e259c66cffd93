// api_checks.hpp — the pointer checks the C-ABI exports share: 16-byte alignment, and whether the
// buffers of one call overlap. Host only and free of HIP: nothing is dereferenced, addresses are
// compared as integers (tests/cpp/api_checks_driver.cpp builds it with the host compiler alone).
#pragma once
#include <cstddef>
#include <cstdint>

namespace mrt {

// Rays, states, guides and colours move as 16-byte words.
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// A buffer argument: its start and the bytes the call reads or writes there.
struct Span {
    const void* p;
    int64_t bytes;
};

// Whether two buffers share a byte. A null pointer or a non-positive length shares none. The
// distance between the starts is set against the lower buffer's length: no start + bytes is formed,
// so a bogus pointer near the top of the address space cannot wrap the sum.
inline bool overlap(const Span& a, const Span& b) {
    if (!a.p || !b.p || a.bytes <= 0 || b.bytes <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a0 <= b0 ? b0 - a0 < static_cast<uint64_t>(a.bytes) : a0 - b0 < static_cast<uint64_t>(b.bytes);
}

// Does an output overlap an input?
template <size_t NI, size_t NO>
bool output_overlaps_input(const Span (&ins)[NI], const Span (&outs)[NO]) {
    for (const Span& out : outs)
        for (const Span& in : ins)
            if (overlap(out, in)) return true;
    return false;
}

// Do two outputs overlap?
template <size_t NO>
bool outputs_overlap(const Span (&outs)[NO]) {
    for (size_t i = 0; i < NO; i++)
        for (size_t j = i + 1; j < NO; j++)
            if (overlap(outs[i], outs[j])) return true;
    return false;
}

// No output may overlap an input or another output.
template <size_t NI, size_t NO>
bool any_overlap(const Span (&ins)[NI], const Span (&outs)[NO]) {
    return output_overlaps_input(ins, outs) || outputs_overlap(outs);
}

}  // namespace mrt
