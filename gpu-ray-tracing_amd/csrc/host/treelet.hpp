// treelet.hpp — treelet restructuring of a Compact2 node array on the host (treelet.cpp): the
// CPU statement of the device's (csrc/treelet_kernel.hip), the arithmetic treelet_common.hpp's
// on both sides. Depends on nothing else, so tests/cpp/treelet_driver.cpp builds it alone.
#pragma once
#include <cstdint>

namespace mrt {

constexpr int kOptimizeMaxRounds = 8;

struct OptimizeStats {
    int32_t rounds = 0;
    int32_t levels = 0;                           // height levels after the last round
    int64_t considered[kOptimizeMaxRounds] = {};  // records of height >= 1, per round
    int64_t rewritten[kOptimizeMaxRounds] = {};   // treelets whose records were rewritten, per round
};

// rounds (1..kOptimizeMaxRounds) passes over numNodes records at nodes, in place. Each pass takes
// the height levels of the tree as it stands (mrt_refit_plan's: a leaf-only record has height 0)
// and runs treelet::restructure on every record of a level before the next level up; height 0
// has nothing to do. Returns nullptr, or why the records are not a tree (nothing written).
const char* optimize_nodes(int32_t* nodes, int64_t numNodes, int rounds, OptimizeStats* stats);

}  // namespace mrt
