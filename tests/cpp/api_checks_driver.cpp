// api_checks_driver.cpp — the C-ABI's pointer checks (csrc/api_checks.hpp) run on made-up addresses
// (tests/test_api_checks.py). Host compiler, no HIP, no library: that it compiles is the test that
// the header is HIP-free. No address is dereferenced.
//
//   aligned A                          -> "aligned 0|1"
//   overlap A bytesA B bytesB          -> "overlap 0|1 0|1"          (a, b) and (b, a)
//   table (in bytes) x3 (out bytes) x3 -> "table oi=0|1 oo=0|1 any=0|1"
//
// Addresses are unsigned (any base strtoull reads), lengths signed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gpu-ray-tracing_amd/csrc/api_checks.hpp"

namespace {

int at = 1, count = 0;
char** words = nullptr;

const char* next() {
    if (at >= count) {
        std::fprintf(stderr, "api_checks_driver: an op is short of numbers\n");
        std::exit(2);
    }
    return words[at++];
}

const void* address() {
    return reinterpret_cast<const void*>(static_cast<uintptr_t>(std::strtoull(next(), nullptr, 0)));
}

mrt::Span span() {
    const void* p = address();
    return mrt::Span{p, static_cast<int64_t>(std::strtoll(next(), nullptr, 0))};
}

}  // namespace

int main(int argc, char** argv) {
    count = argc;
    words = argv;
    while (at < count) {
        const char* op = next();
        if (!std::strcmp(op, "aligned")) {
            std::printf("aligned %d\n", (int)mrt::aligned16(address()));
        } else if (!std::strcmp(op, "overlap")) {
            const mrt::Span a = span(), b = span();
            std::printf("overlap %d %d\n", (int)mrt::overlap(a, b), (int)mrt::overlap(b, a));
        } else if (!std::strcmp(op, "table")) {
            const mrt::Span ins[] = {span(), span(), span()};
            const mrt::Span outs[] = {span(), span(), span()};
            std::printf("table oi=%d oo=%d any=%d\n", (int)mrt::output_overlaps_input(ins, outs), (int)mrt::outputs_overlap(outs),
                        (int)mrt::any_overlap(ins, outs));
        } else {
            std::fprintf(stderr, "api_checks_driver: unknown op %s\n", op);
            return 2;
        }
    }
    return 0;
}
