// Node rows -> the dense [G, k, F] tensor of a batch of graphs (include/tfgx_rows3d.h, where the layout is written down):
// utils.convert_x_to_3d (plain mode) and the SortPool readout nn.sort_pool_3d (sort mode), ONE launch each.
//
// Reference: tf_geometric/utils/graph_utils.py:215-249, nn/pool/sort_pool.py:7-35, nn/pool/topk_pool.py:6-87.
//
// One workgroup per graph.  Sort mode: the ranking of tfgx_static_pool_select, restated here (its kernel keeps its bits): the
// graph's (descending_bits(key) << 32 | position) keys go to LDS, every node's rank is the number of keys below its own — the
// keys are distinct, so the ranks are a permutation and ties fall in plan order.  Each thread holds kSelItems keys in registers
// and streams the LDS keys past them (one broadcast ds_read_b64 serves kSelItems compares of all 256 lanes).  The nodes of the
// first min(n, k) ranks are staged in LDS (16 KiB); the same workgroup then copies their rows, a wave to a row, and zero-fills the
// other rows of the graph.  Behind the graphs, the fill workgroups: -1 for node_slot of the nodes no graph lists; the first of
// them is the ONE writer of the flag word.  No atomics: every output is a pure function of the inputs.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "tfgx_topk_keys.h"
#include "../../include/tfgx_pool_static.h"
#include "../../include/tfgx_rows3d.h"

namespace tfgx {
namespace {

constexpr int kMaxGraph = TFGX_STATIC_POOL_MAX_GRAPH_NODES;
constexpr int kSelItems = 4;                           // keys a thread ranks per pass over the LDS keys
constexpr int kFillTile = kBlock * 4;                  // positions per workgroup of the fill section
constexpr int kWavesPerBlock = kBlock / kWave;
static_assert(kMaxGraph % (kBlock * kSelItems) == 0, "the cap is a whole number of ranking passes");
static_assert(TFGX_ROWS3D_TOO_LONG == TFGX_STATIC_POOL_TOO_LONG, "the flag is ORed into counts[3] of a static batch");

using compact::clampi;

struct Rows3dParams {
    const int32_t* seg_ptr;
    const int32_t* seg_node;
    int32_t G, N, n_rows, F, k;
    const float* x;
    int64_t ldx;
    const float* key;
    int64_t ldkey;
    float* out;
    int64_t ldo;
    int32_t* slot_node;
    int32_t* node_slot;
    int32_t* flags;
    int32_t vec;                       // 16-byte accesses: ldx, ldo and both bases allow them
};

// the node at plan position pos (pos < N), held to the rows of x
__device__ __forceinline__ int32_t node_at(const Rows3dParams& p, int32_t pos)
{
    return p.seg_node != nullptr ? clampi(p.seg_node[pos], 0, p.n_rows - 1) : pos;
}

// out row `orow` = x row `node` (live) or zeros, by the lanes of one wave
__device__ __forceinline__ void copy_row(const Rows3dParams& p, int64_t orow, int32_t node, bool live, int lane)
{
    float* __restrict__ dst = p.out + orow * p.ldo;
    const int32_t F4 = p.vec ? p.F / 4 : 0;
    if (live) {                                         // wave-uniform
        const float* __restrict__ src = p.x + int64_t(node) * p.ldx;
        for (int32_t q = lane; q < F4; q += kWave) {
            float v[4];
            load_vec<4>(src + 4 * q, v);
            store_vec<4>(dst + 4 * q, v);
        }
        for (int32_t c0 = 4 * F4; c0 < p.F; c0 += kWave) {
            const int32_t c = c0 + lane;
            const float v = src[min(c, p.F - 1)];       // the column is clamped; the mask is on the store side only
            if (c < p.F) dst[c] = v;
        }
    } else {
        const float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int32_t q = lane; q < F4; q += kWave) store_vec<4>(dst + 4 * q, z);
        for (int32_t c = 4 * F4 + lane; c < p.F; c += kWave) dst[c] = 0.0f;
    }
}

template <bool SORT>
__global__ void __launch_bounds__(kBlock) rows3d_kernel(const Rows3dParams p)
{
    __shared__ uint64_t keys[SORT ? kMaxGraph : 1];     // 32 KiB
    __shared__ int32_t sel[SORT ? kMaxGraph : 1];       // 16 KiB: rank -> node, for the ranks that have a slot
    const int32_t b = int32_t(blockIdx.x);
    if (b >= p.G) {                                     // ---- the fill section
        int32_t lo = 0, hi = 0;
        if (p.G > 0) {
            lo = clampi(p.seg_ptr[0], 0, p.N);
            hi = clampi(p.seg_ptr[p.G], lo, p.N);
        }
#pragma unroll
        for (int it = 0; it < kFillTile / kBlock; ++it) {
            const int64_t pos = int64_t(b - p.G) * kFillTile + it * kBlock + threadIdx.x;
            if (pos >= p.n_rows || (pos >= lo && pos < hi)) continue;
            // seg_node covers [0, N) and N == n_rows with it; without it the position is the node
            p.node_slot[node_at(p, int32_t(pos))] = -1;
        }
        if (b == p.G && p.flags != nullptr) {           // the one writer of the flag word
            int any = 0;
            if (SORT)
                for (int32_t g = threadIdx.x; g < p.G; g += kBlock) {
                    const int32_t r0 = clampi(p.seg_ptr[g], 0, p.N), r1 = clampi(p.seg_ptr[g + 1], r0, p.N);
                    any |= (r1 - r0 > kMaxGraph) ? 1 : 0;
                }
            any = __syncthreads_or(any);
            if (threadIdx.x == 0) *p.flags = any ? TFGX_ROWS3D_TOO_LONG : 0;
        }
        return;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int32_t r0 = clampi(p.seg_ptr[b], 0, p.N), r1 = clampi(p.seg_ptr[b + 1], r0, p.N);
    const int32_t n = r1 - r0;
    const int64_t slot0 = int64_t(b) * p.k;             // (G * k fits int32)
    int32_t m = min(n, p.k);                            // the slots that hold a node
    if (SORT) {
        if (n > kMaxGraph) {                            // flagged by the fill section; no node has a slot (workgroup-uniform)
            for (int32_t i = threadIdx.x; i < n; i += kBlock) p.node_slot[node_at(p, r0 + i)] = -1;
            m = 0;
        } else {
            for (int32_t i = threadIdx.x; i < n; i += kBlock)
                keys[i] = (uint64_t(descending_bits(p.key[int64_t(node_at(p, r0 + i)) * p.ldkey])) << 32) | uint32_t(i);
            __syncthreads();
            for (int32_t i0 = 0; i0 < n; i0 += kBlock * kSelItems) {
                uint64_t mine[kSelItems];
                int32_t below[kSelItems];
#pragma unroll
                for (int t = 0; t < kSelItems; ++t) {
                    const int32_t i = i0 + t * kBlock + int32_t(threadIdx.x);
                    mine[t] = i < n ? keys[i] : 0;      // key 0 has nothing below it
                    below[t] = 0;
                }
                for (int32_t j = 0; j < n; ++j) {
                    const uint64_t kj = keys[j];        // one address for the whole wave: a broadcast read
#pragma unroll
                    for (int t = 0; t < kSelItems; ++t) below[t] += kj < mine[t] ? 1 : 0;
                }
#pragma unroll
                for (int t = 0; t < kSelItems; ++t) {
                    const int32_t i = i0 + t * kBlock + int32_t(threadIdx.x);
                    if (i >= n) continue;
                    const int32_t node = node_at(p, r0 + i);
                    const bool keep = below[t] < m;     // rank = below[t] < n <= kMaxGraph
                    if (keep) {
                        sel[below[t]] = node;
                        p.slot_node[slot0 + below[t]] = node;
                    }
                    p.node_slot[node] = keep ? int32_t(slot0 + below[t]) : -1;
                }
            }
            __syncthreads();                            // sel is complete
        }
    } else {
        for (int32_t i = threadIdx.x; i < n; i += kBlock) {
            const int32_t node = node_at(p, r0 + i);
            if (i < m) p.slot_node[slot0 + i] = node;
            p.node_slot[node] = i < m ? int32_t(slot0 + i) : -1;
        }
    }
    for (int32_t j = m + int32_t(threadIdx.x); j < p.k; j += kBlock) p.slot_node[slot0 + j] = -1;
    if (p.F == 0) return;
    for (int32_t j = wave; j < p.k; j += kWavesPerBlock) {
        const bool live = j < m;
        int32_t node = 0;
        if (live) node = SORT ? sel[j] : node_at(p, r0 + j);
        copy_row(p, slot0 + j, node, live, lane);
    }
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_rows3d_version(void) { return TFGX_ROWS3D_ABI_VERSION; }

extern "C" int tfgx_segment_rows_3d_f32(const int32_t* seg_ptr, const int32_t* seg_node, int64_t G, int64_t N, const float* x,
                                        int64_t ldx, int64_t n_rows, int64_t F, int64_t k, const float* key, int64_t ldkey,
                                        float* out, int64_t ldo, int32_t* slot_node, int32_t* node_slot, int32_t* flags,
                                        tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const char* fn = "tfgx_segment_rows_3d_f32";
    if (int rc = check_size(fn, "G", G)) return rc;
    if (int rc = check_size(fn, "N", N)) return rc;
    if (int rc = check_size(fn, "n_rows", n_rows)) return rc;
    if (int rc = check_size(fn, "F", F)) return rc;
    if (k < 1) return bad_arg(fn, "k must be at least 1", k);
    if (int rc = check_size(fn, "k", k)) return rc;
    if (G * k >= kMaxSize) {                            // both factors are below 2^31: no overflow
        set_error("%s: G * k = %lld slots do not fit int32 (G = %lld, k = %lld)", fn, (long long)(G * k), (long long)G, (long long)k);
        return TFGX_ERR_INVALID_ARG;
    }
    if (ldx < F) return bad_arg(fn, "ldx is smaller than F", ldx);
    if (ldo < F) return bad_arg(fn, "ldo is smaller than F", ldo);
    if (key != nullptr && ldkey < 1) return bad_arg(fn, "ldkey must be at least 1 with a key", ldkey);
    if (N > n_rows) {
        set_error("%s: N = %lld positions are more than n_rows = %lld", fn, (long long)N, (long long)n_rows);
        return TFGX_ERR_INVALID_ARG;
    }
    if (seg_node != nullptr && N != n_rows) {
        set_error("%s: seg_node lists every node once, but N = %lld is not n_rows = %lld", fn, (long long)N, (long long)n_rows);
        return TFGX_ERR_INVALID_ARG;
    }
    if (G == 0 && n_rows == 0) return TFGX_OK;
    if (G > 0 && seg_ptr == nullptr) return null_arg(fn, "seg_ptr");
    if (G > 0 && N > 0 && F > 0 && x == nullptr) return null_arg(fn, "x");
    if (G > 0 && F > 0 && out == nullptr) return null_arg(fn, "out");
    if (G > 0 && slot_node == nullptr) return null_arg(fn, "slot_node");
    if (n_rows > 0 && node_slot == nullptr) return null_arg(fn, "node_slot");
    if (key != nullptr && flags == nullptr) return null_arg(fn, "flags");

    Rows3dParams p = {};
    p.seg_ptr = seg_ptr, p.seg_node = seg_node;
    p.G = int32_t(G), p.N = int32_t(N), p.n_rows = int32_t(n_rows), p.F = int32_t(F), p.k = int32_t(k);
    p.x = x, p.ldx = ldx, p.key = key, p.ldkey = ldkey, p.out = out, p.ldo = ldo;
    p.slot_node = slot_node, p.node_slot = node_slot, p.flags = flags;
    p.vec = (ldx % 4 == 0 && ldo % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 16)) ? 1 : 0;
    const int64_t fill_tiles = max(int64_t(1), (n_rows + kFillTile - 1) / kFillTile);
    if (G + fill_tiles >= kMaxSize) return bad_arg(fn, "G graphs and the fill tiles of n_rows exceed one grid", G + fill_tiles);
    const unsigned grid = static_cast<unsigned>(G + fill_tiles);
    if (key != nullptr) rows3d_kernel<true><<<grid, kBlock, 0, as_stream(stream_)>>>(p);
    else rows3d_kernel<false><<<grid, kBlock, 0, as_stream(stream_)>>>(p);
    TFGX_LAUNCH_CHECK("rows3d_kernel");
    return TFGX_OK;
}
