// live_key_common.hpp — the live-first sort key of a block of a frame's secondary rays: the
// arithmetic shared verbatim by block_live_kernel (csrc/shard_kernel.hip, hipcc) and
// tests/cpp/frame_plan_driver.cpp, which runs it on the CPU against mrt.dist.live_priority,
// the host's restatement (KEY_MAX = 4094 = kKeyMax - 1 there).
#pragma once
#include <cstdint>

#include "frame_limits.hpp"

#if defined(__HIPCC__)
#define MRT_LIVE_KEY_HD __host__ __device__
#else
#define MRT_LIVE_KEY_HD
#endif

namespace mrt {
namespace frame {

// The key of a block of blockRays rays of which `live` will be traced (their primary ray hit):
// decreasing live = increasing key, so a stable ascending sort puts the fullest blocks first.
// Blocks above kKeyMax - 1 rays are quantized to 12 bits, rounding up (only a block with every
// ray live gets key 0). The frame's partial last block gets the largest key: it sorts last.
MRT_LIVE_KEY_HD inline int live_first_key(int blockRays, int live, bool partial) {
    int key = blockRays - live;
    if (blockRays > kKeyMax - 1) key = (int)(((int64_t)key * (kKeyMax - 1) + blockRays - 1) / blockRays);
    if (partial) key = kKeyMax;
    return key;
}

}  // namespace frame
}  // namespace mrt
