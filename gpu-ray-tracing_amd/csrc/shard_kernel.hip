// shard_kernel.hip — the multi-GPU shard order on the device (gfx950): a rank's blocks of a
// frame's secondary-ray order (block i to rank i % world), listed in frame order or sorted
// live-first, and their launch functions (shard_kernel.hpp). The C-ABI that calls them is
// frame_api.cpp (mrt_shard_blocks). Nothing here waits on the host, and no workgroup ever waits
// for another.
//
// The sort is a stable LSD radix sort of 12-bit keys in LDS by 1024-thread workgroups:
// block_order_kernel holds a whole list of at most kOrderMax entries in 98 KB of static LDS,
// block_tile_sort_kernel one tile of a longer list in 114 KB (+ its key histogram), so the file
// builds for gfx950's 160 KB per workgroup only (the static_assert below says so).
//
// The kernels take their arguments by value as the file-local structs below; ShardArgs adds
// nothing to the launch interface's ShardLaunch: a kernel's mangled symbol is then the one it had
// before the interface existed, so profiles and assembly diffs against older builds match by name.
#include "shard_kernel.hpp"

#include "frame_limits.hpp"
#include "live_key_common.hpp"

namespace mrt {
namespace {

using namespace frame;

// A list of at most kOrderMax blocks: two launches (longer lists: the tile kernels below):
//   block_live_kernel   one wave per listed block: its live rays = the samples of its input
//                       rays whose primary hit (RayGenKernels.cu:117-227: a missed primary's
//                       samples get tmax = -1), as the sort key B - live (the frame's partial
//                       last block: the largest key, so it sorts last);
//   block_order_kernel  one workgroup: a stable LSD radix sort of the list by that key in LDS
//                       (three 4-bit digit passes; per-thread digit counts over contiguous chunks
//                       keep equal keys in list = frame order), then the ordered block ids.
struct ShardArgs : ShardLaunch {};

__device__ inline int shard_block_id(const ShardArgs& a, int j) { return a.rank + j * a.world; }

__global__ __launch_bounds__(kThreads) void block_live_kernel(ShardArgs a) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t jj = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);   // one wave per entry
    if (jj >= a.numBlocks) return;
    const int j = (int)jj;
    const int64_t g0 = (int64_t)shard_block_id(a, j) * a.blockRays;
    const int64_t g1 = min(g0 + a.blockRays, a.totalRays);
    const int64_t p0 = g0 / a.numSamples, p1 = (g1 - 1) / a.numSamples;   // input rays touching the block
    int live = 0;
    for (int64_t p = p0 + lane; p <= p1; p += 64) {
        if (a.results[2 * p].x >= 0) {
            const int64_t lo = max(g0, p * a.numSamples), hi = min(g1, (p + 1) * a.numSamples);
            live += (int)(hi - lo);
        }
    }
    for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
    // mrt.dist.live_priority restates the key on the host
    if (lane == 0) a.out[j] = live_first_key(a.blockRays, live, g1 - g0 < a.blockRays);
}

// Inclusive prefix sum over a wave's 64 lanes in six DPP adds (row_shr 1/2/4/8 within each
// 16-lane row, then row_bcast 15/31 across rows): VALU only, no LDS permutes.
__device__ inline int wave_scan_incl(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

constexpr int kOrderWaves = kOrderThreads / 64;
#if defined(__HIP_DEVICE_COMPILE__)
constexpr int kOrderLdsBytes = 3 * kOrderMax * (int)sizeof(uint16_t) + 2 * kOrderWaves * 16 * (int)sizeof(int);
constexpr int kTileLdsBytes = kOrderLdsBytes + (kKeyMax + 1) * (int)sizeof(int);   // + block_tile_sort_kernel's histogram
#if defined(__gfx950__)
constexpr int kDeviceLdsBytes = 160 * 1024;
#else
constexpr int kDeviceLdsBytes = 64 * 1024;
#endif
static_assert(kTileLdsBytes <= kDeviceLdsBytes,
              "mrt_shard_blocks' LDS sort (block_order_kernel, block_tile_sort_kernel) holds 16384 list entries in "
              "about 98-114 KB of static LDS: it needs gfx950's 160 KB per workgroup, and this device target has "
              "64 KB - build with ARCH=gfx950");
#endif

// The stable sort of n <= kOrderMax list entries in LDS, by all of one workgroup's threads:
// key[i] and idx[0][i] = i are set (not yet synchronised); on return idx[src][0..n) is the
// order (src returned; the caller synchronises before it reads another thread's entries).
__device__ __forceinline__ int order_tile_in_lds(uint16_t* key, uint16_t (*idx)[kOrderMax],
                                                 int (*waveTot)[16], int (*wavePre)[16], int n) {
    constexpr int kWaves = kOrderWaves;
    static_assert((16 * kWaves) % 64 == 0, "the prefix wave walks (digit, wave) entries 64 at a time");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = (n + kOrderThreads - 1) / kOrderThreads;
    const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
    int src = 0;
    for (int shift = 0; shift < 12; shift += 4, src ^= 1) {
        __syncthreads();
        // this thread's digit counts over its contiguous chunk of the current order (registers:
        // the digit selects by compare, no dynamic register indexing)
        int c[16];
#pragma unroll
        for (int e = 0; e < 16; e++) c[e] = 0;
        for (int i = lo; i < hi; i++) {
            const int d = (key[idx[src][i]] >> shift) & 15;
#pragma unroll
            for (int e = 0; e < 16; e++) c[e] += d == e;
        }
        // exclusive offsets in (digit, thread) order: digit totals before d, plus this digit's
        // counts of the threads before t — a wave scan per digit, the waves' totals through LDS,
        // their (digit, wave) exclusive prefix by one wave, read back once per digit
        int pre[16];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int v = wave_scan_incl(c[e]);
            pre[e] = v - c[e];
            if (lane == 63) waveTot[wave][e] = v;
        }
        __syncthreads();
        if (wave == 0) {   // lane l < 16 * kWaves / 64 ... one entry (digit e, wave w) per step, in order
            int run = 0;
            for (int e0 = 0; e0 < 16 * kWaves; e0 += 64) {
                const int q = e0 + lane, e = q / kWaves, w = q - e * kWaves;
                const int v = waveTot[w][e];
                const int incl = wave_scan_incl(v);
                wavePre[w][e] = run + incl - v;
                run += __builtin_amdgcn_readlane(incl, 63);
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e++) pre[e] += wavePre[wave][e];
        for (int i = lo; i < hi; i++) {
            const uint16_t v = idx[src][i];
            const int d = (key[v] >> shift) & 15;
            int pos = 0;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                pos = d == e ? pre[e] : pos;
                pre[e] += d == e;
            }
            idx[src ^ 1][pos] = v;
        }
    }
    return src;
}

__global__ __launch_bounds__(kOrderThreads) void block_order_kernel(ShardArgs a) {
    __shared__ uint16_t key[kOrderMax];
    __shared__ uint16_t idx[2][kOrderMax];
    __shared__ int waveTot[kOrderWaves][16];
    __shared__ int wavePre[kOrderWaves][16];
    const int t = (int)threadIdx.x, n = a.numBlocks;
    for (int i = t; i < n; i += kOrderThreads) {
        key[i] = (uint16_t)a.out[i];
        idx[0][i] = (uint16_t)i;
    }
    const int src = order_tile_in_lds(key, idx, waveTot, wavePre, n);
    __syncthreads();
    for (int i = t; i < n; i += kOrderThreads) a.out[i] = shard_block_id(a, idx[src][i]);
}

// Lists longer than kOrderMax (mrt_shard_blocks): three launches after block_live_kernel, each
// a phase that reads what every workgroup of the one before wrote — the stream orders them;
// no workgroup ever waits for another.
//   block_tile_sort_kernel     workgroup = one tile of <= kOrderMax consecutive list entries:
//                              the LDS sort above; the tile-sorted (key, index in tile) pairs to
//                              pairs[], the tile's counts per key — read off the run boundaries
//                              of the sorted keys — to table[key][tile];
//   block_hist_scan_kernel     one workgroup: table -> its exclusive prefix sum in memory order,
//                              key-major, tile-minor = where each tile's run of each key starts
//                              in the sorted list (equal keys: lower tile first, so list order);
//   block_tile_scatter_kernel  workgroup = tile: entry i of the tile's order, of key k, goes to
//                              table[k][tile] + (i - the run's first i), as its block id.
// The keys stay in the list until block_tile_sort_kernel has read them; only the scatter
// writes block ids there.
struct TileArgs {
    ShardArgs s;
    uint32_t* pairs;   // [s.numBlocks]: key << 16 | index in tile, tile-sorted
    int32_t* table;    // [kKeyMax + 1][numTiles]
    int numTiles;
};

__global__ __launch_bounds__(kOrderThreads) void block_tile_sort_kernel(TileArgs a) {
    __shared__ uint16_t key[kOrderMax];
    __shared__ uint16_t idx[2][kOrderMax];
    __shared__ int waveTot[kOrderWaves][16];
    __shared__ int wavePre[kOrderWaves][16];
    __shared__ int count[kKeyMax + 1];
    const int t = (int)threadIdx.x, tile = (int)blockIdx.x;
    const int64_t base = (int64_t)tile * kOrderMax;
    const int n = (int)min((int64_t)kOrderMax, (int64_t)a.s.numBlocks - base);   // the last tile is short
    if (tile >= a.numTiles || n <= 0) return;                                   // workgroup-uniform
    for (int i = t; i < n; i += kOrderThreads) {
        key[i] = (uint16_t)(a.s.out[base + i] & kKeyMax);
        idx[0][i] = (uint16_t)i;
    }
    for (int k = t; k <= kKeyMax; k += kOrderThreads) count[k] = 0;
    const int src = order_tile_in_lds(key, idx, waveTot, wavePre, n);
    __syncthreads();
    const uint16_t* ord = idx[src];
    for (int i = t; i < n; i += kOrderThreads) {   // a run's last entry: its end
        const int v = ord[i], k = key[v];
        a.pairs[base + i] = (uint32_t)k << 16 | (uint32_t)v;
        if (i + 1 == n || key[ord[i + 1]] != k) count[k] = i + 1;
    }
    __syncthreads();
    for (int i = t; i < n; i += kOrderThreads) {   // a run's first entry: end - start
        const int k = key[ord[i]];
        if (i == 0 || key[ord[i - 1]] != k) count[k] -= i;
    }
    __syncthreads();
    for (int k = t; k <= kKeyMax; k += kOrderThreads) a.table[(int64_t)k * a.numTiles + tile] = count[k];
}

// In place; numTiles rounds of 4 * kOrderThreads = kKeyMax + 1 consecutive entries (so no
// ragged end), one int4 per thread, the next round's load issued before this round's barriers.
__global__ __launch_bounds__(kOrderThreads) void block_hist_scan_kernel(int32_t* table, int numTiles) {
    static_assert(4 * kOrderThreads == kKeyMax + 1, "a round is one int4 per thread");
    __shared__ int waveTot[kOrderWaves];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    int4* tv = reinterpret_cast<int4*>(table);
    int carry = 0;
    int4 next = numTiles > 0 ? tv[t] : make_int4(0, 0, 0, 0);
    for (int r = 0; r < numTiles; r++) {
        const int4 v = next;
        if (r + 1 < numTiles) next = tv[(int64_t)(r + 1) * kOrderThreads + t];
        const int sum = v.x + v.y + v.z + v.w;
        const int incl = wave_scan_incl(sum);
        if (lane == 63) waveTot[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kOrderWaves; w++) {
            const int x = waveTot[w];
            all += x;
            before += w < wave ? x : 0;
        }
        const int ex = carry + before + incl - sum;
        tv[(int64_t)r * kOrderThreads + t] = make_int4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
        carry += all;
        __syncthreads();   // waveTot is rewritten next round
    }
}

__global__ __launch_bounds__(kOrderThreads) void block_tile_scatter_kernel(TileArgs a) {
    __shared__ int first[kKeyMax + 1];   // per key of the tile: its run's place in the list - its first i
    const int t = (int)threadIdx.x, tile = (int)blockIdx.x;
    const int64_t base = (int64_t)tile * kOrderMax;
    const int n = (int)min((int64_t)kOrderMax, (int64_t)a.s.numBlocks - base);
    if (tile >= a.numTiles || n <= 0) return;
    for (int i = t; i < n; i += kOrderThreads) {
        const int k = (int)(a.pairs[base + i] >> 16) & kKeyMax;
        if (i == 0 || ((int)(a.pairs[base + i - 1] >> 16) & kKeyMax) != k)
            first[k] = a.table[(int64_t)k * a.numTiles + tile] - i;
    }
    __syncthreads();
    for (int i = t; i < n; i += kOrderThreads) {
        const uint32_t p = a.pairs[base + i];
        const int64_t pos = (int64_t)first[(int)(p >> 16) & kKeyMax] + i;   // every run's first entry set first[]
        const int64_t j = base + (int)(p & 0xFFFF);
        if (pos >= 0 && pos < a.s.numBlocks && j < a.s.numBlocks) a.s.out[pos] = shard_block_id(a.s, (int)j);
    }
}

__global__ __launch_bounds__(kThreads) void block_list_kernel(ShardArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < a.numBlocks) a.out[j] = shard_block_id(a, (int)j);
}

}  // namespace

hipError_t launch_shard_list(const ShardLaunch& a, int grid, hipStream_t s) {
    hipLaunchKernelGGL(block_list_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, ShardArgs{a});
    return hipGetLastError();
}

hipError_t launch_shard_order(const ShardLaunch& a, int liveGrid, hipStream_t s) {
    hipLaunchKernelGGL(block_live_kernel, dim3((unsigned)liveGrid), dim3(kThreads), 0, s, ShardArgs{a});
    hipLaunchKernelGGL(block_order_kernel, dim3(1), dim3(kOrderThreads), 0, s, ShardArgs{a});
    return hipGetLastError();
}

hipError_t launch_shard_order_tiled(const ShardLaunch& a, int liveGrid, int numTiles, int32_t* table, uint32_t* pairs,
                                    hipStream_t s) {
    TileArgs ta{};
    ta.s = ShardArgs{a};
    ta.pairs = pairs;
    ta.table = table;
    ta.numTiles = numTiles;
    hipLaunchKernelGGL(block_live_kernel, dim3((unsigned)liveGrid), dim3(kThreads), 0, s, ta.s);
    hipLaunchKernelGGL(block_tile_sort_kernel, dim3((unsigned)numTiles), dim3(kOrderThreads), 0, s, ta);
    hipLaunchKernelGGL(block_hist_scan_kernel, dim3(1), dim3(kOrderThreads), 0, s, table, numTiles);
    hipLaunchKernelGGL(block_tile_scatter_kernel, dim3((unsigned)numTiles), dim3(kOrderThreads), 0, s, ta);
    return hipGetLastError();
}

}  // namespace mrt
