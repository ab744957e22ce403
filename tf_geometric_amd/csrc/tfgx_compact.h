// The device bodies the graph builders share: order-stable tile compaction, the one-workgroup exclusive scan, and the small
// wave helpers around them.  tfgx_subgraph.hip, tfgx_dropedge.hip and tfgx_pool_static.hip compact with the tile pair below,
// tfgx_pool_static.hip and tfgx_collate_static.hip scan their tables with block_exclusive_scan.
//
// Tile compaction: a launch of kBlock threads per tile of kTile items; thread t owns items tile_item(0 .. kTileItems).
//   count : tile_count leaves the kept items of every tile in tile_cnt; the caller scans them into tile_off.
//   emit  : item i = base + it * kBlock + wave * 64 + lane lands at
//           tile_off[tile] + (kept items of earlier (it, wave) slots of the tile) + (kept lanes below it in its wave).
// What is kept, what is stored and any guard on the store belong to the caller: the helpers take callables.
#pragma once
#include "tfgx_common.h"

namespace tfgx {
namespace compact {

constexpr int kTileItems = 8;                          // items per thread per tile
constexpr int kTile = kBlock * kTileItems;             // 2048 items per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kScanBlock = 1024;                       // threads of the one-workgroup scan
constexpr int kScanWaves = kScanBlock / kWave;

inline int64_t num_tiles(int64_t n) { return (n + kTile - 1) / kTile; }

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return max(lo, min(v, hi)); }

// set bits of `mask` in the lanes below this one
__device__ __forceinline__ int lane_prefix(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0));
}

// the bits of a wave ballot of `keep` that belong to this lane's sub-group of G lanes (G | 64), moved down to bit 0
template <int G>
__device__ __forceinline__ uint64_t group_bits(bool keep)
{
    const int lane = threadIdx.x & (kWave - 1);
    return (__ballot(keep) >> (lane - lane % G)) & ((G == 64) ? ~uint64_t(0) : ((uint64_t(1) << G) - 1));
}

// item `it` of this thread in tile blockIdx.x
__device__ __forceinline__ int64_t tile_item(int it) { return int64_t(blockIdx.x) * kTile + it * kBlock + threadIdx.x; }

// tile_cnt[blockIdx.x] = the items i of the tile with keep(i).  One barrier.
template <class Keep>
__device__ __forceinline__ void tile_count(Keep keep, int32_t* __restrict__ tile_cnt)
{
    __shared__ int32_t wave_cnt[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int cnt = 0;
#pragma unroll
    for (int it = 0; it < kTileItems; ++it) cnt += __popcll(__ballot(keep(tile_item(it))));
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) t += wave_cnt[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// mask[it] = the wave's ballot of "item `it` is kept".  For every it, emit(it, first, pos): `first` is the output position of
// the first kept item of this wave's 64 items, `pos` the position of this lane's own item — meaningful where it is kept.
template <class Emit>
__device__ __forceinline__ void tile_positions(const uint64_t (&mask)[kTileItems], const int32_t* __restrict__ tile_off, Emit emit)
{
    __shared__ int32_t slot_cnt[kTileItems][kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int it = 0; it < kTileItems; ++it)
        if (lane == 0) slot_cnt[it][wave] = __popcll(mask[it]);
    __syncthreads();
    int32_t off = tile_off[blockIdx.x];
#pragma unroll
    for (int it = 0; it < kTileItems; ++it) {
        int32_t before = 0, total = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) {
            const int32_t c = slot_cnt[it][w];
            before += (w < wave) ? c : 0;
            total += c;
        }
        emit(it, off + before, off + before + lane_prefix(mask[it]));
        off += total;
    }
}

// ---- the one-workgroup scan: kScanBlock threads, thread t owns the contiguous slots [begin, end) of n ----------------------
struct Run {
    int32_t begin, end;
};

__device__ __forceinline__ Run thread_run(int32_t n)
{
    const int32_t per = (n + kScanBlock - 1) / kScanBlock;
    const int32_t begin = int32_t(min(int64_t(n), int64_t(threadIdx.x) * per));
    return Run{begin, int32_t(min(int64_t(n), int64_t(begin) + per))};
}

__device__ __forceinline__ int64_t shfl_up(int64_t v, int off) { return __shfl_up(static_cast<long long>(v), off, kWave); }

// exclusive prefix of `v` over the kScanBlock threads; `total` = the sum over all of them.  T supplies +, - and shfl_up, and
// T{} is its zero.  Wave scans with shuffles, the 16 wave totals through LDS.  Two barriers.
template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T& total)
{
    __shared__ T wave_total[kScanWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    T inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T up = shfl_up(inc, off);
        if (lane >= off) inc = inc + up;
    }
    if (lane == kWave - 1) wave_total[wave] = inc;
    __syncthreads();
    T base = T{};
    total = T{};
    for (int w = 0; w < kScanWaves; ++w) {
        const T t = wave_total[w];
        if (w < wave) base = base + t;
        total = total + t;
    }
    __syncthreads();                                    // wave_total is free again
    return base + inc - v;
}

}  // namespace compact
}  // namespace tfgx
