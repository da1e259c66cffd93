// deal_common.hpp — which ray a lane of a one-shot launch traces (cfg.oneshot): the index
// arithmetic shared verbatim by the launch plan (csrc/launch_plan.cpp, g++), the one-shot
// kernels (csrc/trace_kernel.hip, hipcc) and tests/cpp/deal_driver.cpp, which enumerates it
// on the CPU.
//
// A one-shot grid is a backfilled static grid (launch_plan.hpp) in which every lane takes at
// most one ray. The workgroups with equal blockIdx % 8 form a group (one XCD under the
// round-robin placement: a speed assumption only, as in the strided rounds). Each group
// owns c positions:
//   b = 0   the contiguous chunk [g c, (g + 1) c) of the batch, c = roundup64(ceil(n / 8)):
//           what the first strided round of a backfilled grid deals today;
//   b >= 6  the 2^b-ray blocks g, g + 8, g + 16, ... of the batch, c = ceil(ceil(n / 2^b) / 8)
//           blocks: position p is ray (((p >> b) * 8 + g) << b) | (p & (2^b - 1)), the queue
//           modes' block-cyclic share (trace_kernel.hip, queueBlockLog2). Every group then
//           samples the whole Morton-ordered frame, so the groups cost alike.
// A position's ray may lie past the batch (the last blocks): that lane has no ray.
// Within a group the positions go to lanes as in the strided rounds: consecutive 64-position
// tiles to different workgroups (wave w of the group's workgroup j takes tile
// w * blocksPerGroup + j), and with 2^k lane groups the G = 64 >> k lanes of group s take G
// consecutive positions of the s-th 2^k-th of the chunk.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MRT_DEAL_HD __host__ __device__
#else
#define MRT_DEAL_HD
#endif

namespace mrt {
namespace deal {

constexpr int kGroups = 8;
constexpr int kMinBlockLog2 = 6, kMaxBlockLog2 = 15;

// Positions per group, a multiple of 64. n <= 2^30 rays: 8 c <= n + 8 * 2^15 stays inside int32.
MRT_DEAL_HD inline int chunk(int n, int b) {
    if (b == 0) return ((n + kGroups - 1) / kGroups + 63) & ~63;
    const int blocks = (int)(((int64_t)n + (1 << b) - 1) >> b);
    return ((blocks + kGroups - 1) / kGroups) << b;
}

// Workgroups per group of the grid that gives every position of a chunk a lane.
MRT_DEAL_HD inline int blocks_per_group(int c, int blockThreads) { return (c + blockThreads - 1) / blockThreads; }

// The position in its group's chunk of lane `lane` of wave `wave` of the group's workgroup j
// (blockIdx / 8); >= c: the lane has none.
MRT_DEAL_HD inline int position(int c, int blocksPerGroup, int j, int wave, int lane, int laneGroupsLog2) {
    const int tile = wave * blocksPerGroup + j;
    const int local = tile * 64 + lane;
    if (local >= c || laneGroupsLog2 <= 0) return local;
    const int gl = 6 - laneGroupsLog2;   // log2 lanes per lane group
    const int sg = lane >> gl, p = lane & ((1 << gl) - 1);
    return ((sg * (c >> 6) + tile) << gl) + p;
}

// The ray of position p (< c) of group g; >= n: no ray.
MRT_DEAL_HD inline int ray(int p, int g, int c, int b) {
    if (b == 0) return g * c + p;
    return ((((p >> b) * kGroups) + g) << b) | (p & ((1 << b) - 1));
}

// The ray of a lane of workgroup `block` of a one-shot grid over n rays; n: no ray.
MRT_DEAL_HD inline int lane_ray(int n, int b, int laneGroupsLog2, int blocksPerGroup, int block, int wave, int lane) {
    const int c = chunk(n, b);
    const int p = position(c, blocksPerGroup, block / kGroups, wave, lane, laneGroupsLog2);
    if (p >= c) return n;
    const int r = ray(p, block % kGroups, c, b);
    return r < n ? r : n;
}

}  // namespace deal
}  // namespace mrt
