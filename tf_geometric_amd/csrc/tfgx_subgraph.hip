// Node-induced subgraph + the row gathers of SAGPool / SortPool.
//
// Reference: BatchGraph.sample_new_graph_by_node_index (tf_geometric/data/graph.py:276-359) with
// compute_edge_mask_by_node_index (utils/graph_utils.py:538-551): keep the edges whose two endpoints are both in the
// kept-node list, renumber them by position in that list, carry edge attributes along.  Here:
//   count : node_map[n] (new id or -1, duplicates / out-of-range ids flagged), per-tile kept-edge counts, one scan;
//           the host reads {kept count, flags} in ONE device -> host copy.
//   emit  : order-stable compaction (the tile scheme of tfgx_compact.h, tile offsets from the scan) of the relabelled edge list and
//           the original id of every kept edge; optionally the pooled graph's CSR plan DERIVED from the parent plan:
//           tfgx_build_csr_by_dst is a stable sort by destination, so the kept edges of parent row node_index[j], walked
//           in CSR order, are pooled row j in the order a rebuild would produce — no sort.
// Gather-scale rows (x[idx] * s[idx]) and its backward (one row per wave over ALL parent rows through node_map: no
// memset, no atomics, fixed-order reduction).  Integer atomics only (flags, duplicate detection); never on floats.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "tfgx_gather.h"
#include <hipcub/hipcub.hpp>

namespace tfgx {
namespace {

using namespace compact;

// node_map[v] = -1 for every node; tile_cnt[nt] = 0 (the scan's extra entry that becomes the total)
__global__ void node_map_fill(int32_t* __restrict__ node_map, int64_t n, int32_t* __restrict__ tile_cnt_end)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    if (i == 0) *tile_cnt_end = 0;
    for (; i < n; i += stride) node_map[i] = -1;
}

// node_map[node_index[i]] = i; a second claim of the same node or an id outside [0, n) sets flags[0]
__global__ void node_map_scatter(const int32_t* __restrict__ node_index, int64_t m, int64_t n,
                                 int32_t* __restrict__ node_map, int32_t* __restrict__ flags)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    int bad = 0;
    for (; i < m; i += stride) {
        const int32_t v = node_index[i];
        if (v < 0 || v >= n) {
            bad = 1;
            continue;
        }
        bad |= atomicCAS(node_map + v, -1, int32_t(i)) != -1;
    }
    if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flags, 1);
}

// kept-edge count of every tile of kTile edges; an endpoint outside [0, n) sets flags[1]
__global__ void __launch_bounds__(kBlock) edge_tile_count(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                          int64_t E, int64_t n, const int32_t* __restrict__ node_map,
                                                          int32_t* __restrict__ tile_cnt, int32_t* __restrict__ flags)
{
    int bad = 0;
    tile_count(
        [&](int64_t e) {
            if (e >= E) return false;
            const int32_t r = row[e], c = col[e];
            const bool ok = (r >= 0) & (r < n) & (c >= 0) & (c < n);
            bad |= !ok;
            return ok && node_map[r] >= 0 && node_map[c] >= 0;
        },
        tile_cnt);
    if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flags + 1, 1);
}

// The order-stable compaction of tfgx_compact.h over the edges.  The store has NO `pos < n_kept` guard: the positions come from
// this call's own count pass over the same node_map.
__global__ void __launch_bounds__(kBlock) edge_tile_emit(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                         int64_t E, const int32_t* __restrict__ node_map,
                                                         const int32_t* __restrict__ tile_off,
                                                         int32_t* __restrict__ out_row, int32_t* __restrict__ out_col,
                                                         int32_t* __restrict__ out_edge_id, int32_t* __restrict__ rank)
{
    uint64_t mask[kTileItems];
    int32_t nr[kTileItems], nc[kTileItems];
#pragma unroll
    for (int it = 0; it < kTileItems; ++it) {
        const int64_t e = tile_item(it);
        nr[it] = -1;
        nc[it] = -1;
        if (e < E) {          // endpoints were validated by the count pass
            nr[it] = node_map[row[e]];
            nc[it] = node_map[col[e]];
        }
        mask[it] = __ballot((nr[it] >= 0) & (nc[it] >= 0));
    }
    tile_positions(mask, tile_off, [&](int it, int32_t, int32_t pos) {
        if ((nr[it] >= 0) & (nc[it] >= 0)) {
            const int64_t e = tile_item(it);
            out_row[pos] = nr[it];
            out_col[pos] = nc[it];
            out_edge_id[pos] = int32_t(e);
            if (rank != nullptr) rank[e] = pos;
        }
    });
}

// G lanes per pooled row j (G | 64): walk parent row node_index[j] in CSR order, count the edges whose source is kept
template <int G>
__global__ void __launch_bounds__(kBlock) plan_row_count(const int32_t* __restrict__ p_row_ptr, const int32_t* __restrict__ p_col,
                                                         const int32_t* __restrict__ node_index, int64_t m,
                                                         const int32_t* __restrict__ node_map, int32_t* __restrict__ cnt)
{
    const int lig = threadIdx.x % G;
    const int64_t groups = int64_t(gridDim.x) * (kBlock / G);
    for (int64_t j = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / G; j < m; j += groups) {
        const int32_t o = node_index[j];
        const int32_t s = p_row_ptr[o], t = p_row_ptr[o + 1];
        int32_t c = 0;
        for (int32_t b = s; b < t; b += G) {
            const int32_t p = b + lig;
            c += __popcll(group_bits<G>(p < t && node_map[p_col[p]] >= 0));
        }
        if (lig == 0) cnt[j] = c;
    }
}

template <int G>
__global__ void __launch_bounds__(kBlock) plan_row_emit(const int32_t* __restrict__ p_row_ptr, const int32_t* __restrict__ p_col,
                                                        const int32_t* __restrict__ p_perm,
                                                        const int32_t* __restrict__ node_index, int64_t m,
                                                        const int32_t* __restrict__ node_map, const int32_t* __restrict__ rank,
                                                        int64_t E, const int32_t* __restrict__ n_kept,
                                                        const int32_t* __restrict__ row_ptr, int32_t* __restrict__ col_out,
                                                        int32_t* __restrict__ perm_out)
{
    // a parent plan of ANOTHER edge list (the caller's mistake) must not write past the n_kept outputs nor read past rank
    const int32_t cap = *n_kept;
    const int lig = threadIdx.x % G;
    const uint64_t below = (uint64_t(1) << lig) - 1;
    const int64_t groups = int64_t(gridDim.x) * (kBlock / G);
    for (int64_t j = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / G; j < m; j += groups) {
        const int32_t o = node_index[j];
        const int32_t s = p_row_ptr[o], t = p_row_ptr[o + 1];
        int32_t pos = row_ptr[j];
        for (int32_t b = s; b < t; b += G) {
            const int32_t p = b + lig;
            int32_t nc = -1;
            if (p < t) nc = node_map[p_col[p]];
            const uint64_t bits = group_bits<G>(nc >= 0);
            if (nc >= 0) {
                const int32_t q = pos + __popcll(bits & below);
                const int32_t pe = p_perm[p];
                if (q < cap) {
                    col_out[q] = nc;
                    perm_out[q] = (pe >= 0 && pe < E) ? rank[pe] : -1;
                }
            }
            pos += __popcll(bits);
        }
    }
}

// One wave per PARENT row o: j = node_map[o];  dx[o,:] = j >= 0 ? g[j,:] * s[o] : 0;  ds[o] = j >= 0 ? sum_f g[j,f] x[o,f] : 0.
// Lane l accumulates items l, l + 64, ... in order; the wave sum is a fixed xor butterfly: bit-reproducible.
__global__ void __launch_bounds__(kBlock) gather_scale_backward(const float* __restrict__ g, int64_t ldg,
                                                                const int32_t* __restrict__ node_map, int64_t n,
                                                                const float* __restrict__ x, int64_t ldx,
                                                                const float* __restrict__ s, int64_t F, int64_t F4,
                                                                float* __restrict__ dx, int64_t lddx, float* __restrict__ ds)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t W = F4 + (F - 4 * F4);
    const int64_t waves = int64_t(gridDim.x) * kWavesPerBlock;
    for (int64_t o = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave; o < n; o += waves) {
        const int64_t j = node_map[o];
        const float sc = (j >= 0 && s != nullptr) ? s[o] : 1.0f;
        float acc = 0.0f;
        for (int64_t q = lane; q < W; q += kWave) {
            if (q < F4) {
                float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (j >= 0) load_vec<4>(g + j * ldg + 4 * q, gv);
                if (dx != nullptr) {
                    float d[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) d[k] = gv[k] * sc;
                    store_vec<4>(dx + o * lddx + 4 * q, d);
                }
                if (ds != nullptr && j >= 0) {
                    float xv[4];
                    load_vec<4>(x + o * ldx + 4 * q, xv);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc = fmaf(gv[k], xv[k], acc);
                }
            } else {
                const int64_t c = 4 * F4 + (q - F4);
                const float gv = j >= 0 ? g[j * ldg + c] : 0.0f;
                if (dx != nullptr) dx[o * lddx + c] = gv * sc;
                if (ds != nullptr && j >= 0) acc = fmaf(gv, x[o * ldx + c], acc);
            }
        }
        if (ds != nullptr) {
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
            if (lane == 0) ds[o] = acc;
        }
    }
}

struct Layout {
    int64_t nt;
    size_t off_tile_cnt, off_tile_off, off_row_cnt, off_rank, off_temp, temp_bytes, total;
};

// Workspace: [tile_cnt (nt + 1) | tile_off (nt + 1), flags (2) | row_cnt (m + 1) | rank (E) | scan temp]; the last two
// row_cnt / rank only with a plan.  tile_off is followed directly by the two flag words, so tile_off[nt] (the kept-edge
// total) and the flags are ONE contiguous 12-byte block, fetched with a single device -> host copy.
Layout layout(int64_t n, int64_t E, int64_t m, int with_plan)
{
    (void)n;
    Layout L;
    L.nt = num_tiles(E);
    const size_t scan_tiles = scan_bytes(L.nt + 1), scan_rows = with_plan ? scan_bytes(m + 1) : 0;
    L.temp_bytes = align256(scan_tiles > scan_rows ? scan_tiles : scan_rows);
    L.off_tile_cnt = 0;
    L.off_tile_off = align256(sizeof(int32_t) * size_t(L.nt + 1));
    L.off_row_cnt = L.off_tile_off + align256(sizeof(int32_t) * size_t(L.nt + 3));
    L.off_rank = L.off_row_cnt + (with_plan ? align256(sizeof(int32_t) * size_t(m + 1)) : 0);
    L.off_temp = L.off_rank + (with_plan ? align256(sizeof(int32_t) * size_t(E > 0 ? E : 1)) : 0);
    L.total = L.off_temp + L.temp_bytes;
    return L;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" size_t tfgx_induced_subgraph_workspace_bytes(int64_t n, int64_t E, int64_t m, int32_t with_plan)
{
    if (n < 0 || E < 0 || m < 0) return 0;
    return layout(n, E, m, with_plan).total;
}

extern "C" int tfgx_induced_subgraph_count(const int32_t* row, const int32_t* col, int64_t E, int64_t n,
                                           const int32_t* node_index, int64_t m, int32_t* node_map, int64_t* n_kept,
                                           void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    TFGX_REQUIRE(E >= 0 && n >= 0 && m >= 0, "negative size");
    TFGX_REQUIRE(E < (int64_t(1) << 31) - 1 && n < (int64_t(1) << 31) - 1 && m < (int64_t(1) << 31) - 1,
                 "sizes must fit int32");
    TFGX_REQUIRE(n_kept != nullptr, "n_kept (host) is null");
    TFGX_REQUIRE(workspace != nullptr, "workspace is null");
    TFGX_REQUIRE((n == 0 || node_map) && (m == 0 || node_index) && (E == 0 || (row && col)), "null pointer");
    const Layout lay = layout(n, E, m, 0);
    if (workspace_bytes < lay.total) {
        set_error("tfgx_induced_subgraph_count: workspace too small (%zu < %zu)", workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    int32_t* tile_cnt = reinterpret_cast<int32_t*>(ws + lay.off_tile_cnt);
    int32_t* tile_off = reinterpret_cast<int32_t*>(ws + lay.off_tile_off);
    int32_t* flags = tile_off + lay.nt + 1;

    TFGX_HIP_CHECK(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream));
    node_map_fill<<<grid_for(n, kBlock), kBlock, 0, stream>>>(node_map, n, tile_cnt + lay.nt);
    TFGX_LAUNCH_CHECK("node_map_fill");
    if (m > 0) {
        node_map_scatter<<<grid_for(m, kBlock), kBlock, 0, stream>>>(node_index, m, n, node_map, flags);
        TFGX_LAUNCH_CHECK("node_map_scatter");
    }
    if (E > 0) {
        edge_tile_count<<<static_cast<unsigned>(lay.nt), kBlock, 0, stream>>>(row, col, E, n, node_map, tile_cnt, flags);
        TFGX_LAUNCH_CHECK("edge_tile_count");
    }
    size_t tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.off_temp, tb, tile_cnt, tile_off, static_cast<int>(lay.nt + 1),
                                                    stream));
    int32_t host[3] = {0, 0, 0};      // {kept edges, bad node_index, bad edge endpoint}
    TFGX_HIP_CHECK(hipMemcpyAsync(host, tile_off + lay.nt, sizeof(host), hipMemcpyDeviceToHost, stream));
    TFGX_HIP_CHECK(hipStreamSynchronize(stream));
    if (host[1]) {
        set_error("tfgx_induced_subgraph_count: node_index holds a duplicate or an id outside [0, %lld)", (long long)n);
        return TFGX_ERR_INVALID_ARG;
    }
    if (host[2]) {
        set_error("tfgx_induced_subgraph_count: edge endpoint outside [0, %lld)", (long long)n);
        return TFGX_ERR_INDEX;
    }
    *n_kept = host[0];
    return TFGX_OK;
}

extern "C" int tfgx_induced_subgraph_emit(const int32_t* row, const int32_t* col, int64_t E, int64_t n,
                                          const int32_t* node_index, int64_t m, const int32_t* node_map, int64_t n_kept,
                                          const int32_t* parent_row_ptr, const int32_t* parent_col,
                                          const int32_t* parent_perm, int32_t* out_row, int32_t* out_col,
                                          int32_t* out_edge_id, int32_t* out_row_ptr, int32_t* out_plan_col,
                                          int32_t* out_plan_perm, void* workspace, size_t workspace_bytes,
                                          tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    TFGX_REQUIRE(E >= 0 && n >= 0 && m >= 0, "negative size");
    TFGX_REQUIRE(E < (int64_t(1) << 31) - 1 && n < (int64_t(1) << 31) - 1 && m < (int64_t(1) << 31) - 1,
                 "sizes must fit int32");
    const int with_plan = parent_row_ptr != nullptr;
    TFGX_REQUIRE(with_plan == (out_row_ptr != nullptr), "parent_row_ptr and out_row_ptr go together");
    TFGX_REQUIRE(n_kept >= 0 && n_kept <= E, "n_kept outside [0, E]");
    TFGX_REQUIRE(!with_plan || E == 0 || (parent_col && parent_perm), "plan: null parent pointer");
    TFGX_REQUIRE(!with_plan || n_kept == 0 || (out_plan_col && out_plan_perm), "plan: null output pointer");
    TFGX_REQUIRE(workspace != nullptr, "workspace is null");
    TFGX_REQUIRE((n == 0 || node_map) && (m == 0 || node_index) && (E == 0 || (row && col)), "null pointer");
    TFGX_REQUIRE(n_kept == 0 || (out_row && out_col && out_edge_id), "null output pointer");
    const Layout lay = layout(n, E, m, with_plan);
    if (workspace_bytes < lay.total) {
        set_error("tfgx_induced_subgraph_emit: workspace too small (%zu < %zu)", workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    const int32_t* tile_off = reinterpret_cast<const int32_t*>(ws + lay.off_tile_off);
    int32_t* rank = with_plan ? reinterpret_cast<int32_t*>(ws + lay.off_rank) : nullptr;
    if (n_kept > 0) {
        edge_tile_emit<<<static_cast<unsigned>(lay.nt), kBlock, 0, stream>>>(row, col, E, node_map, tile_off, out_row,
                                                                              out_col, out_edge_id, rank);
        TFGX_LAUNCH_CHECK("edge_tile_emit");
    }
    if (!with_plan) return TFGX_OK;
    int32_t* row_cnt = reinterpret_cast<int32_t*>(ws + lay.off_row_cnt);
    TFGX_HIP_CHECK(hipMemsetAsync(row_cnt + m, 0, sizeof(int32_t), stream));
    // short rows (graph batches: a few edges per node) share a wave 8 to a row; long rows get a wave each
    const bool wide = n > 0 && E / n > 16;
    if (m > 0) {
        if (wide) {
            plan_row_count<64><<<grid_for(m, kBlock / 64), kBlock, 0, stream>>>(parent_row_ptr, parent_col, node_index, m,
                                                                                node_map, row_cnt);
        } else {
            plan_row_count<8><<<grid_for(m, kBlock / 8), kBlock, 0, stream>>>(parent_row_ptr, parent_col, node_index, m,
                                                                              node_map, row_cnt);
        }
        TFGX_LAUNCH_CHECK("plan_row_count");
    }
    size_t tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.off_temp, tb, row_cnt, out_row_ptr, static_cast<int>(m + 1),
                                                    stream));
    if (m > 0 && n_kept > 0) {
        if (wide) {
            plan_row_emit<64><<<grid_for(m, kBlock / 64), kBlock, 0, stream>>>(parent_row_ptr, parent_col, parent_perm,
                                                                               node_index, m, node_map, rank, E, tile_off + lay.nt,
                                                                               out_row_ptr, out_plan_col, out_plan_perm);
        } else {
            plan_row_emit<8><<<grid_for(m, kBlock / 8), kBlock, 0, stream>>>(parent_row_ptr, parent_col, parent_perm,
                                                                             node_index, m, node_map, rank, E, tile_off + lay.nt,
                                                                             out_row_ptr, out_plan_col, out_plan_perm);
        }
        TFGX_LAUNCH_CHECK("plan_row_emit");
    }
    return TFGX_OK;
}

extern "C" int tfgx_gather_i32(const int32_t* src, const int32_t* idx, int64_t M, int32_t* dst, tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(M >= 0, "negative size");
    if (M == 0) return TFGX_OK;
    TFGX_REQUIRE(src && idx && dst, "null pointer");
    gather_by_index<<<grid_for(M, kBlock), kBlock, 0, as_stream(stream)>>>(src, idx, M, dst);
    TFGX_LAUNCH_CHECK("gather_by_index");
    return TFGX_OK;
}

extern "C" int tfgx_gather_scale_rows_f32(const float* x, int64_t ldx, const int32_t* idx, const float* s, int64_t M,
                                          int64_t F, float* out, int64_t ldo, tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(M >= 0 && F >= 0 && ldx >= F && ldo >= F, "bad size / leading dimension");
    if (M == 0 || F == 0) return TFGX_OK;
    TFGX_REQUIRE(x && idx && out, "null pointer");
    const bool vec = ldx % 4 == 0 && ldo % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 16);
    const int64_t F4 = vec ? F / 4 : 0;
    gather_scale_rows<false><<<grid_for(M * (F4 + F - 4 * F4), kBlock), kBlock, 0, as_stream(stream)>>>(x, ldx, 0, idx, s, M, F,
                                                                                                        F4, out, ldo);
    TFGX_LAUNCH_CHECK("gather_scale_rows");
    return TFGX_OK;
}

extern "C" int tfgx_gather_scale_rows_backward_f32(const float* g, int64_t ldg, const int32_t* node_map, int64_t n,
                                                   const float* x, int64_t ldx, const float* s, int64_t F, float* dx,
                                                   int64_t lddx, float* ds, tfgx_stream_t stream)
{
    TFGX_RANGE();
    TFGX_REQUIRE(n >= 0 && F >= 0 && ldg >= F, "bad size / leading dimension");
    TFGX_REQUIRE(dx == nullptr || lddx >= F, "bad lddx");
    TFGX_REQUIRE(ds == nullptr || (x != nullptr && ldx >= F), "ds needs x");
    if (n == 0 || (dx == nullptr && ds == nullptr)) return TFGX_OK;
    TFGX_REQUIRE(node_map != nullptr && (F == 0 || g != nullptr), "null pointer");
    const bool vec = ldg % 4 == 0 && aligned_to(g, 16) && (dx == nullptr || (lddx % 4 == 0 && aligned_to(dx, 16))) &&
                     (ds == nullptr || (ldx % 4 == 0 && aligned_to(x, 16)));
    const int64_t F4 = vec ? F / 4 : 0;
    gather_scale_backward<<<grid_for(n, kWavesPerBlock), kBlock, 0, as_stream(stream)>>>(g, ldg, node_map, n, x, ldx, s, F,
                                                                                          F4, dx, lddx, ds);
    TFGX_LAUNCH_CHECK("gather_scale_backward");
    return TFGX_OK;
}
