// host_error.hpp — the thread-local text behind mrth_last_error, shared by the files that define
// mrt_host.h's functions (host_api.cpp, raysort.cpp).
#pragma once
#include <string>

namespace mrt {

// Remembers msg for mrth_last_error and returns code.
int host_fail(int code, const std::string& msg);
const char* host_last_error();

}  // namespace mrt
