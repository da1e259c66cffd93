// trace_limits.hpp — limits of a trace launch that the kernels (trace_kernel.hpp), the launch
// configuration (launch_plan.cpp) and the autotuner (tune.cpp) all read. Plain C++, no HIP.
#pragma once

namespace mrt {

constexpr int kMaxQueues = 8;   // per-XCD ray queues of one launch (cfg.num_queues), one head each

}  // namespace mrt
