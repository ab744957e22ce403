// Device-side builders of the per-plan structures the fast routes read: walk order, hub chunk lists, hub_order_slot and
// the source-block partition of a CSR plan — what tf_geometric_amd/plan.py used to assemble from torch ops (argsort,
// nonzero / cumsum / repeat_interleave, searchsorted, an int64-key argsort + bincount).  Every output is fully determined
// by row_ptr and col, so no builder sorts where a stable partition or a scan suffices:
//   walk order    : degree max -> host skew test (one sync) -> stable descending radix sort of (degree, row id)
//                   (hipcub, plumbing only; only on skewed plans).
//   hub lists     : per-span flag / chunk count, two scans, one sync for the totals; emit = one thread per hub row
//                   (rows, chunk_ptr) + one thread per chunk (binary search for its row).
//   order slot    : one binary search per hub row.
//   source blocks : ONE wave per destination row, no sort, no workspace: pass 1 counts the row's edges per block (lane b
//                   owns block b's counter), a wave scan turns the counts into rpk, pass 2 writes col_k in place with the
//                   ballot + lane_prefix of tfgx_compact.h, order-stable (per distinct block in a 64-edge chunk: one
//                   ballot, one readlane of the block's cursor).  col is read twice (the second read mostly from cache),
//                   col_k written once, rpk once.
// Integer atomics only (the degree maximum); never on floats.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include <hipcub/hipcub.hpp>
#include <cmath>

namespace tfgx {
namespace {

constexpr int kWavesPerBlockP = kBlock / kWave;
constexpr int kMaxSourceBlocks = 64;                    // one lane per block of a row

inline int value_bits(int64_t v)
{
    int b = 1;
    while (b < 31 && (int64_t(1) << b) <= v) ++b;
    return b;
}

// ---- walk order ---------------------------------------------------------------------------------------------------
// deg[r] = row_ptr[r + 1] - row_ptr[r], iota[r] = r, *max_deg = max over rows (integer atomic, one per wave)
__global__ void degree_iota_max(const int32_t* __restrict__ row_ptr, int64_t n, uint32_t* __restrict__ deg,
                                int32_t* __restrict__ iota, int32_t* __restrict__ max_deg)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    int32_t m = 0;
    for (; i < n; i += stride) {
        const int32_t d = row_ptr[i + 1] - row_ptr[i];
        deg[i] = static_cast<uint32_t>(d > 0 ? d : 0);
        iota[i] = static_cast<int32_t>(i);
        m = d > m ? d : m;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(m, off, kWave);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && m > 0) atomicMax(max_deg, m);
}

// ---- hub lists ----------------------------------------------------------------------------------------------------
// span r = [row_begin[r * s], row_end[r * s]); flag[r] = its length > threshold, nch[r] = its chunk count (0 if no hub)
__global__ void hub_flag_count(const int32_t* __restrict__ row_begin, const int32_t* __restrict__ row_end, int64_t s,
                               int64_t n, int32_t threshold, int32_t chunk, int32_t* __restrict__ flag,
                               int64_t* __restrict__ nch)
{
    int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; r < n; r += stride) {
        const int64_t len = int64_t(row_end[r * s]) - int64_t(row_begin[r * s]);
        const bool hub = len > threshold;
        flag[r] = hub ? 1 : 0;
        nch[r] = hub ? (len + chunk - 1) / chunk : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {     // the scans' extra entries that become the totals
        flag[n] = 0;
        nch[n] = 0;
    }
}

// totals[0] = hub rows, totals[1] = chunks: one contiguous 16-byte device -> host read
__global__ void hub_totals(const int32_t* __restrict__ hub_pos, const int64_t* __restrict__ chunk_off, int64_t n,
                           int64_t* __restrict__ totals)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = hub_pos[n];
        totals[1] = chunk_off[n];
    }
}

__global__ void hub_emit_rows(const int32_t* __restrict__ flag, const int32_t* __restrict__ hub_pos,
                              const int64_t* __restrict__ chunk_off, int64_t n, int64_t n_hub,
                              int32_t* __restrict__ rows, int32_t* __restrict__ chunk_ptr)
{
    int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; r < n; r += stride) {
        if (flag[r]) {
            const int32_t i = hub_pos[r];
            if (i < n_hub) {        // a span changed between _count and _emit must not write past the counted outputs
                rows[i] = static_cast<int32_t>(r);
                chunk_ptr[i] = static_cast<int32_t>(chunk_off[r]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) chunk_ptr[n_hub] = static_cast<int32_t>(chunk_off[n]);
}

// chunk c belongs to hub row i = (last i with chunk_ptr[i] <= c); it covers [begin + k * chunk, min(+chunk, end))
__global__ void hub_emit_chunks(const int32_t* __restrict__ row_begin, const int32_t* __restrict__ row_end, int64_t s,
                                int64_t n_rows, const int32_t* __restrict__ rows, const int32_t* __restrict__ chunk_ptr,
                                int64_t n_hub, int64_t n_chunks, int32_t chunk, int32_t* __restrict__ chunk_begin,
                                int32_t* __restrict__ chunk_end, int32_t* __restrict__ chunk_row)
{
    int64_t c = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; c < n_chunks; c += stride) {
        int64_t lo = 0, hi = n_hub;             // upper_bound(chunk_ptr[0 .. n_hub), c) - 1
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (chunk_ptr[mid] <= c) lo = mid + 1;
            else hi = mid;
        }
        const int64_t i = lo > 0 ? lo - 1 : 0;
        const int32_t r = rows[i];
        if (r < 0 || r >= n_rows) continue;     // only if the spans changed since _count: read nothing outside them
        const int64_t b0 = row_begin[int64_t(r) * s], e0 = row_end[int64_t(r) * s];
        const int64_t b = b0 + (c - chunk_ptr[i]) * int64_t(chunk);
        const int64_t e = b + chunk < e0 ? b + chunk : e0;
        chunk_begin[c] = static_cast<int32_t>(b);
        chunk_end[c] = static_cast<int32_t>(e);
        chunk_row[c] = r;
    }
}

// slot[i] = lower_bound(hub_rows[0 .. n_hub), order[i]) for i < n_hub
__global__ void hub_order_slot_kernel(const int32_t* __restrict__ hub_rows, int64_t n_hub,
                                      const int32_t* __restrict__ order, int32_t* __restrict__ slot)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; i < n_hub; i += stride) {
        const int32_t v = order[i];
        int64_t lo = 0, hi = n_hub;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (hub_rows[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        slot[i] = static_cast<int32_t>(lo);
    }
}

// ---- source blocks ------------------------------------------------------------------------------------------------
// One wave per destination row r.  Lane b (< KB) keeps block b's edge counter (pass 1), then its cursor (pass 2).
// An edge's block is clamped to [0, KB): whatever col holds, every write stays inside the row's own positions.
__global__ void __launch_bounds__(kBlock) source_blocks_kernel(const int32_t* __restrict__ row_ptr,
                                                               const int32_t* __restrict__ col, int64_t n_dst, int64_t E,
                                                               int32_t KB, int64_t blk, int32_t* __restrict__ rpk,
                                                               int32_t* __restrict__ col_k)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = int64_t(gridDim.x) * kWavesPerBlockP;
    const uint64_t below = (uint64_t(1) << lane) - 1;
    for (int64_t r = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave; r < n_dst; r += waves) {
        const int32_t s = row_ptr[r], t = row_ptr[r + 1];
        int32_t cnt = 0;
        for (int64_t base = s; base < t; base += kWave) {
            const int64_t p = base + lane;
            int32_t bb = 0;
            if (p < t) {
                const int64_t q = int64_t(col[p]) / blk;
                bb = q < 0 ? 0 : (q >= KB ? KB - 1 : int32_t(q));
            }
            uint64_t pending = __ballot(p < t);
            while (pending) {
                const int b = __builtin_amdgcn_readlane(bb, __builtin_ctzll(pending));
                const uint64_t m = pending & __ballot(bb == b);
                if (lane == b) cnt += __popcll(m);
                pending &= ~m;
            }
        }
        // exclusive prefix over the lanes: cursor of block b = row start + edges of blocks < b
        int32_t inc = cnt;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int32_t o = __shfl_up(inc, off, kWave);
            if (lane >= off) inc += o;
        }
        int32_t cursor = s + inc - cnt;
        if (lane < KB) rpk[r * KB + lane] = cursor;
        for (int64_t base = s; base < t; base += kWave) {
            const int64_t p = base + lane;
            int32_t bb = 0, c = 0;
            if (p < t) {
                c = col[p];
                const int64_t q = int64_t(c) / blk;
                bb = q < 0 ? 0 : (q >= KB ? KB - 1 : int32_t(q));
            }
            uint64_t pending = __ballot(p < t);
            while (pending) {
                const int b = __builtin_amdgcn_readlane(bb, __builtin_ctzll(pending));
                const uint64_t m = pending & __ballot(bb == b);
                const int32_t at = __builtin_amdgcn_readlane(cursor, b);
                if ((m >> lane) & 1) {
                    const int64_t pos = int64_t(at) + compact::lane_prefix(m & below);
                    if (pos >= 0 && pos < E) col_k[pos] = c;
                }
                if (lane == b) cursor += __popcll(m);
                pending &= ~m;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) rpk[n_dst * KB] = static_cast<int32_t>(E);
}

struct RowOrderLayout {
    size_t off_max, off_deg, off_deg_out, off_iota, off_temp, temp_bytes, total;
};

RowOrderLayout row_order_layout(int64_t n_dst)
{
    RowOrderLayout L;
    const int n = static_cast<int>(n_dst > 0 ? n_dst : 1);
    size_t temp = 0;
    const uint32_t* kin = nullptr;
    uint32_t* kout = nullptr;
    const int32_t* vin = nullptr;
    int32_t* vout = nullptr;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp, kin, kout, vin, vout, n, 0, 31);
    const size_t a4 = align256(sizeof(int32_t) * size_t(n));
    L.off_max = 0;
    L.off_deg = 256;
    L.off_deg_out = L.off_deg + a4;
    L.off_iota = L.off_deg_out + a4;
    L.off_temp = L.off_iota + a4;
    L.temp_bytes = align256(temp);
    L.total = L.off_temp + L.temp_bytes;
    return L;
}

struct HubLayout {
    size_t off_flag, off_pos, off_nch, off_off, off_totals, off_temp, temp_bytes, total;
};

// [flag (n + 1) | hub_pos (n + 1) | nch (n + 1, int64) | chunk_off (n + 1, int64) | totals (2, int64) | scan temp]
HubLayout hub_layout(int64_t n)
{
    HubLayout L;
    size_t t32 = 0, t64 = 0;
    const int32_t* i32 = nullptr;
    int32_t* o32 = nullptr;
    const int64_t* i64 = nullptr;
    int64_t* o64 = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t32, i32, o32, static_cast<int>(n + 1));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t64, i64, o64, static_cast<int>(n + 1));
    const size_t a4 = align256(sizeof(int32_t) * size_t(n + 1)), a8 = align256(sizeof(int64_t) * size_t(n + 1));
    L.off_flag = 0;
    L.off_pos = a4;
    L.off_nch = 2 * a4;
    L.off_off = 2 * a4 + a8;
    L.off_totals = 2 * a4 + 2 * a8;
    L.off_temp = L.off_totals + 256;
    L.temp_bytes = align256(t32 > t64 ? t32 : t64);
    L.total = L.off_temp + L.temp_bytes;
    return L;
}

constexpr int64_t kI32Limit = (int64_t(1) << 31) - 1;

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_hub_policy(int64_t E, int64_t n_dst, int32_t* threshold, int32_t* chunk)
{
    TFGX_REQUIRE(E >= 0 && n_dst >= 0, "negative size");
    TFGX_REQUIRE(threshold != nullptr && chunk != nullptr, "threshold / chunk (host) is null");
    const double avg = double(E) / double(n_dst > 1 ? n_dst : 1);
    int32_t thr = 128;
    while (thr < 4.0 * avg && thr < 2048) thr *= 2;
    *threshold = thr;
    *chunk = thr / 2 > 128 ? thr / 2 : 128;
    return TFGX_OK;
}

extern "C" int32_t tfgx_gat_source_block_count(int64_t n_dst, int64_t n_src, int64_t E, int64_t A, int64_t W,
                                               int64_t block_bytes, int64_t min_edges)
{
    if (n_dst < 0 || n_src < 0 || E < 0 || A < 0 || W < 0 || block_bytes < 0 || min_edges < 0) {
        set_error("tfgx_gat_source_block_count: negative argument");
        return 0;
    }
    if (block_bytes == 0) block_bytes = int64_t(6) << 20;
    if (min_edges == 0) min_edges = 32;
    if (n_dst == 0 || E == 0) return 1;
    // nn/conv/gat.py: min(round(table / block_bytes), int(E / n_dst / min_edges), 16) — round() is half-to-even
    const double table = double(n_src * (A + W) * 4);
    const double by_table = std::nearbyint(table / double(block_bytes));
    const double by_edges = std::trunc(double(E) / double(n_dst) / double(min_edges));
    double kb = by_table < by_edges ? by_table : by_edges;
    kb = kb < 16.0 ? kb : 16.0;
    return kb >= 2.0 ? static_cast<int32_t>(kb) : 1;
}

extern "C" size_t tfgx_plan_row_order_workspace_bytes(int64_t n_dst)
{
    if (n_dst < 0) return 0;
    return row_order_layout(n_dst).total;
}

extern "C" int tfgx_plan_row_order(const int32_t* row_ptr, int64_t n_dst, int64_t E, int32_t* order, int32_t* skewed,
                                   void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    TFGX_REQUIRE(n_dst >= 0 && E >= 0, "negative size");
    TFGX_REQUIRE(n_dst < kI32Limit && E < kI32Limit, "sizes must fit int32");
    TFGX_REQUIRE(skewed != nullptr, "skewed (host) is null");
    *skewed = 0;
    if (n_dst == 0 || E == 0) return TFGX_OK;
    TFGX_REQUIRE(row_ptr != nullptr && order != nullptr, "null pointer");
    TFGX_REQUIRE(workspace != nullptr, "workspace is null");
    const RowOrderLayout lay = row_order_layout(n_dst);
    if (workspace_bytes < lay.total) {
        set_error("tfgx_plan_row_order: workspace too small (%zu < %zu)", workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    int32_t* max_deg = reinterpret_cast<int32_t*>(ws + lay.off_max);
    uint32_t* deg = reinterpret_cast<uint32_t*>(ws + lay.off_deg);
    uint32_t* deg_out = reinterpret_cast<uint32_t*>(ws + lay.off_deg_out);
    int32_t* iota = reinterpret_cast<int32_t*>(ws + lay.off_iota);
    TFGX_HIP_CHECK(hipMemsetAsync(max_deg, 0, sizeof(int32_t), stream));
    degree_iota_max<<<grid_for(n_dst, kBlock), kBlock, 0, stream>>>(row_ptr, n_dst, deg, iota, max_deg);
    TFGX_LAUNCH_CHECK("degree_iota_max");
    int32_t m = 0;
    TFGX_HIP_CHECK(hipMemcpyAsync(&m, max_deg, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    TFGX_HIP_CHECK(hipStreamSynchronize(stream));
    // plan.py's skew test: longest row more than 8x the mean (and more than 8 edges)
    const double mean = double(E) / double(n_dst);
    if (!(double(m) > 8.0 * (mean > 1.0 ? mean : 1.0))) return TFGX_OK;
    // the workspace holds a 31-bit sort; the sort runs over the bits of the longest row only (never needs more)
    size_t tb = 0;
    TFGX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, deg, deg_out, iota, order, static_cast<int>(n_dst),
                                                                0, value_bits(m), stream));
    if (tb > lay.temp_bytes) {
        set_error("tfgx_plan_row_order: sort needs %zu temporary bytes, the workspace holds %zu", tb, lay.temp_bytes);
        return TFGX_ERR_WORKSPACE;
    }
    tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairsDescending(ws + lay.off_temp, tb, deg, deg_out, iota, order,
                                                                static_cast<int>(n_dst), 0, value_bits(m), stream));
    *skewed = 1;
    return TFGX_OK;
}

extern "C" size_t tfgx_plan_hub_lists_workspace_bytes(int64_t n_rows)
{
    if (n_rows < 0) return 0;
    return hub_layout(n_rows).total;
}

static int hub_check(const char* fn, const int32_t* row_begin, const int32_t* row_end, int64_t rp_stride, int64_t n_rows,
                     int32_t threshold, int32_t chunk, const void* workspace, size_t workspace_bytes)
{
    if (n_rows < 0 || n_rows >= kI32Limit || rp_stride < 1 || threshold < 0 || chunk < 1) {
        set_error("%s: bad size (n_rows %lld, rp_stride %lld, threshold %d, chunk %d)", fn, (long long)n_rows,
                  (long long)rp_stride, threshold, chunk);
        return TFGX_ERR_INVALID_ARG;
    }
    if (workspace == nullptr || (n_rows > 0 && (row_begin == nullptr || row_end == nullptr))) {
        set_error("%s: null pointer", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    const size_t need = hub_layout(n_rows).total;
    if (workspace_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
        return TFGX_ERR_WORKSPACE;
    }
    return TFGX_OK;
}

extern "C" int tfgx_plan_hub_lists_count(const int32_t* row_begin, const int32_t* row_end, int64_t rp_stride,
                                         int64_t n_rows, int32_t threshold, int32_t chunk, int64_t* n_hub_rows,
                                         int64_t* n_chunks, void* workspace, size_t workspace_bytes,
                                         tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    TFGX_REQUIRE(n_hub_rows != nullptr && n_chunks != nullptr, "n_hub_rows / n_chunks (host) is null");
    const int rc = hub_check(__func__, row_begin, row_end, rp_stride, n_rows, threshold, chunk, workspace, workspace_bytes);
    if (rc != TFGX_OK) return rc;
    const HubLayout lay = hub_layout(n_rows);
    char* ws = static_cast<char*>(workspace);
    int32_t* flag = reinterpret_cast<int32_t*>(ws + lay.off_flag);
    int32_t* pos = reinterpret_cast<int32_t*>(ws + lay.off_pos);
    int64_t* nch = reinterpret_cast<int64_t*>(ws + lay.off_nch);
    int64_t* off = reinterpret_cast<int64_t*>(ws + lay.off_off);
    int64_t* totals = reinterpret_cast<int64_t*>(ws + lay.off_totals);
    hub_flag_count<<<grid_for(n_rows, kBlock), kBlock, 0, stream>>>(row_begin, row_end, rp_stride, n_rows, threshold, chunk,
                                                                     flag, nch);
    TFGX_LAUNCH_CHECK("hub_flag_count");
    size_t tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.off_temp, tb, flag, pos, static_cast<int>(n_rows + 1), stream));
    tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.off_temp, tb, nch, off, static_cast<int>(n_rows + 1), stream));
    hub_totals<<<1, kWave, 0, stream>>>(pos, off, n_rows, totals);
    TFGX_LAUNCH_CHECK("hub_totals");
    int64_t host[2] = {0, 0};
    TFGX_HIP_CHECK(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, stream));
    TFGX_HIP_CHECK(hipStreamSynchronize(stream));
    if (host[1] >= kI32Limit) {
        set_error("tfgx_plan_hub_lists_count: %lld chunks do not fit int32", (long long)host[1]);
        return TFGX_ERR_INVALID_ARG;
    }
    *n_hub_rows = host[0];
    *n_chunks = host[1];
    return TFGX_OK;
}

extern "C" int tfgx_plan_hub_lists_emit(const int32_t* row_begin, const int32_t* row_end, int64_t rp_stride,
                                        int64_t n_rows, int32_t threshold, int32_t chunk, int64_t n_hub_rows,
                                        int64_t n_chunks, int32_t* rows, int32_t* chunk_ptr, int32_t* chunk_begin,
                                        int32_t* chunk_end, int32_t* chunk_row, void* workspace, size_t workspace_bytes,
                                        tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    const int rc = hub_check(__func__, row_begin, row_end, rp_stride, n_rows, threshold, chunk, workspace, workspace_bytes);
    if (rc != TFGX_OK) return rc;
    TFGX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n_rows && n_chunks >= 0 && n_chunks < kI32Limit,
                 "n_hub_rows / n_chunks outside the range _count returns");
    TFGX_REQUIRE(n_hub_rows > 0 || n_chunks == 0, "chunks without hub rows");
    if (n_hub_rows == 0) return TFGX_OK;
    TFGX_REQUIRE(rows && chunk_ptr && (n_chunks == 0 || (chunk_begin && chunk_end && chunk_row)), "null output pointer");
    const HubLayout lay = hub_layout(n_rows);
    char* ws = static_cast<char*>(workspace);
    const int32_t* flag = reinterpret_cast<const int32_t*>(ws + lay.off_flag);
    const int32_t* pos = reinterpret_cast<const int32_t*>(ws + lay.off_pos);
    const int64_t* off = reinterpret_cast<const int64_t*>(ws + lay.off_off);
    hub_emit_rows<<<grid_for(n_rows, kBlock), kBlock, 0, stream>>>(flag, pos, off, n_rows, n_hub_rows, rows, chunk_ptr);
    TFGX_LAUNCH_CHECK("hub_emit_rows");
    if (n_chunks > 0) {
        hub_emit_chunks<<<grid_for(n_chunks, kBlock), kBlock, 0, stream>>>(row_begin, row_end, rp_stride, n_rows, rows, chunk_ptr,
                                                                            n_hub_rows, n_chunks, chunk, chunk_begin,
                                                                            chunk_end, chunk_row);
        TFGX_LAUNCH_CHECK("hub_emit_chunks");
    }
    return TFGX_OK;
}

extern "C" int tfgx_plan_hub_order_slot(const int32_t* hub_rows, int64_t n_hub, const int32_t* order, int32_t* slot,
                                        tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(n_hub >= 0 && n_hub < kI32Limit, "bad n_hub");
    if (n_hub == 0) return TFGX_OK;
    TFGX_REQUIRE(hub_rows && order && slot, "null pointer");
    hub_order_slot_kernel<<<grid_for(n_hub, kBlock), kBlock, 0, as_stream(stream)>>>(hub_rows, n_hub, order, slot);
    TFGX_LAUNCH_CHECK("hub_order_slot_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_plan_source_blocks(const int32_t* row_ptr, const int32_t* col, int64_t n_dst, int64_t n_src, int64_t E,
                                       int32_t KB, int32_t* rpk, int32_t* col_k, tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(n_dst >= 0 && n_src >= 0 && E >= 0, "negative size");
    TFGX_REQUIRE(n_dst < kI32Limit && n_src < kI32Limit && E < kI32Limit, "sizes must fit int32");
    TFGX_REQUIRE(KB >= 1 && KB <= kMaxSourceBlocks, "KB outside [1, 64]");
    TFGX_REQUIRE(rpk != nullptr && (n_dst == 0 || row_ptr != nullptr), "null pointer");
    TFGX_REQUIRE(E == 0 || (col != nullptr && col_k != nullptr), "null pointer");
    const int64_t blk = n_src > 0 ? (n_src + KB - 1) / KB : 1;
    source_blocks_kernel<<<grid_for(n_dst, kWavesPerBlockP), kBlock, 0, as_stream(stream)>>>(row_ptr, col, n_dst, E, KB, blk,
                                                                                             rpk, col_k);
    TFGX_LAUNCH_CHECK("source_blocks_kernel");
    return TFGX_OK;
}
