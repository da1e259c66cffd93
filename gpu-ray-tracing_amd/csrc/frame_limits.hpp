// frame_limits.hpp — the sizes the frame path's kernels (raygen_kernel.hip, shard_kernel.hip) are
// written for and its plan (frame_plan.cpp) sizes grids and scratch by: one copy. Plain C++ with
// no HIP in it; the kernel files pull the names in with a using-directive.
#pragma once

namespace mrt {
namespace frame {

constexpr int kThreads = 256;          // the streaming kernels' workgroup
constexpr int kMaxBatchSeeds = 256;    // batch seeds a launch carries in its arguments
constexpr int kTileRays = 1024;        // output rays of an ao_blocks_tiled_kernel workgroup
constexpr int kOrderThreads = 1024;    // the shard order's sort / scan / scatter workgroup
constexpr int kOrderMax = 16384;       // list entries the one-workgroup sort holds
constexpr int kKeyMax = 4095;          // 12-bit keys
constexpr int kCountBlocks = 1024;     // most partials of a hit count

}  // namespace frame
}  // namespace mrt
