// host_error.cpp — mrth_last_error and the text it returns.
#include "host_error.hpp"

#include "../../../include/mrt_host.h"

namespace mrt {

namespace {
thread_local std::string g_err;
}

int host_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

const char* host_last_error() { return g_err.c_str(); }

}  // namespace mrt

extern "C" const char* mrth_last_error(void) { return mrt::host_last_error(); }
