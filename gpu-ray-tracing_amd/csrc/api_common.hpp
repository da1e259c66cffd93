// api_common.hpp — what the C-ABI files (every *_api.cpp) share on the HIP side: the error returns,
// the device guard, the owners of the device memory, the stream-ordered scratch and the events the
// library allocates, and the outcome of an export's launches. The pointer checks that need no HIP
// are in api_checks.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "../../include/mrt.h"
#include "trace_kernel.hpp"   // api_fail

namespace mrt {

inline int fail(int code, const std::string& what) { return api_fail(code, what); }

inline int hipFail(hipError_t e, const char* what) {
    return fail(MRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define MRT_HIP(call)                                         \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return ::mrt::hipFail(e_, #call); \
    } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// A hipMalloc'ed array of T, freed with its owner (a destructor has nobody to report to: the
// error is dropped). Move-only; a moved-from or default-constructed one holds nothing.
template <class T>
struct DeviceBuf {
    T* p = nullptr;
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) {
            (void)free();
            p = std::exchange(o.p, nullptr);
        }
        return *this;
    }
    ~DeviceBuf() { (void)free(); }
    // `bytes` of new memory in place of what it held; holds nothing when that fails.
    hipError_t alloc(size_t bytes) {
        (void)free();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    hipError_t free() { return p ? hipFree(std::exchange(p, nullptr)) : hipSuccess; }
    T* get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
};

// Stream-ordered scratch of one call (hipMallocAsync): taken on a stream before the launches
// that use it, released on the same stream after the last of them, with no host sync and no
// state shared between calls. release() reports the free's error, for the caller to report
// after a launch's; the destructor frees what an early return left (its error is dropped).
// Move-only.
struct StreamScratch {
    void* p = nullptr;
    hipStream_t stream = nullptr;
    StreamScratch() = default;
    StreamScratch(StreamScratch&& o) noexcept : p(std::exchange(o.p, nullptr)), stream(o.stream) {}
    StreamScratch& operator=(StreamScratch&& o) noexcept {
        if (this != &o) {
            (void)release();
            p = std::exchange(o.p, nullptr);
            stream = o.stream;
        }
        return *this;
    }
    ~StreamScratch() { (void)release(); }
    hipError_t alloc(size_t bytes, hipStream_t s) {
        (void)release();
        stream = s;
        const hipError_t e = hipMallocAsync(&p, bytes, s);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    hipError_t release() { return p ? hipFreeAsync(std::exchange(p, nullptr), stream) : hipSuccess; }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// The outcome of an export's launches.
inline int launched(hipError_t launch, const char* what) { return launch == hipSuccess ? MRT_OK : hipFail(launch, what); }

// The outcome of launches that used stream-ordered scratch: the free is enqueued after them in
// any case, and a launch error is reported in preference to the free's.
inline int launched(hipError_t launch, const char* what, StreamScratch& scratch, const char* whatFree) {
    const hipError_t f = scratch.release();
    if (launch != hipSuccess) return hipFail(launch, what);
    return f == hipSuccess ? MRT_OK : hipFail(f, whatFree);
}

// A hipEvent_t, destroyed with its owner. Move-only.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e = std::exchange(o.e, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    void reset() {
        if (e) (void)hipEventDestroy(std::exchange(e, nullptr));
    }
    operator hipEvent_t() const { return e; }
};

// The events around a timed launch.
struct EventPair {
    Event start, stop;
};

}  // namespace mrt
