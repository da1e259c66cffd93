// path_limits.hpp — the sizes the path frame's kernels (path_kernel.hip) are written for and its
// plan (path_plan.cpp) sizes grids and scratch by: one copy. Plain C++ with no HIP in it.
#pragma once
#include <cstdint>

namespace mrt {
namespace path {

constexpr int kThreads = 256;            // workgroup of the count, extend, accumulate and resolve kernels
constexpr int kWaves = kThreads / 64;    // its waves: the per-wave survivor counts it keeps in LDS
constexpr int kScanThreads = 1024;       // the one scan workgroup: counts it takes in a single round
constexpr int kMaxPaths = 1 << 22;       // slots of one extend / accumulate call (the Renderer's batches: <= 2^21)
constexpr int kMaxDepth = 64;            // bounces of a path: vertices 0..depth
// slots whose workgroup counts fill one round of the scan; one more takes a second round
constexpr int64_t kScanRoundSlots = (int64_t)kScanThreads * kThreads;

}  // namespace path
}  // namespace mrt
