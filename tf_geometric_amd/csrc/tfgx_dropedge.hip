// DropEdge (include/tfgx_dropedge.h): edge dropout as three independent order-stable compactions.
//
// Reference: tf_geometric/nn/sampling/drop_edge.py:6-52.  The keep decision of edge e is drop_hash(seed, e) against the
// rate's threshold (tfgx_common.h; the host restates it as tfgx_dropout_keep), so any array that carries original edge
// ids can be compacted on its own:
//   edge order : (row, col) of the kept edges + their ids              -> out_row / out_col / out_edge_id
//   CSR order  : the parent plan's (col, perm), by destination          -> the dropped list's plan
//   CSR order  : the parent's transposed plan, by source                -> the dropped list's transposed plan
// Every compaction is the tile scheme of tfgx_compact.h: tiles of kTile items, per-tile counts, one scan, then wave
// ballot + mbcnt inside the tile.  Each pass also leaves a GROUP TABLE: per 64 consecutive items {keep bits, kept items
// before the group}, 16 bytes.  rank(i) = table[i / 64].before + popcount(bits below i) then answers
//   new perm[q]    = rank_edge_order(old perm[p])      (the new id of a kept edge)
//   new row_ptr[r] = rank_csr_order(old row_ptr[r])
// with one 16-byte read from a table of E / 4 bytes instead of a gather from an E-sized rank array.  Rows are never
// walked: a row of one edge and a hub of a million take the same path.  Integer atomicOr on the bad-index flag only.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "../../include/tfgx_dropedge.h"
#include <hipcub/hipcub.hpp>

namespace tfgx {
namespace {

using namespace compact;

enum { kEdges = 0, kUpperEdges = 1, kCsr = 2 };

inline int64_t num_groups(int64_t E) { return (E + kWave - 1) / kWave; }

// tfgx_dropout_keep on the device: thr == 0 is "dropout off" (make_drop)
__device__ __forceinline__ bool keep_id(uint32_t thr, uint64_t seed, uint32_t id)
{
    return thr == 0u || (drop_hash(seed, id) >> 8) >= thr;
}

// {keep bits 0-31, keep bits 32-63, kept items before the group, unused}
__device__ __forceinline__ int32_t group_rank(const int4* __restrict__ table, int64_t i)
{
    const int4 g = table[i >> 6];
    const uint64_t bits = (uint64_t(uint32_t(g.y)) << 32) | uint32_t(g.x);
    return g.z + __popcll(bits & ((uint64_t(1) << (i & 63)) - 1));
}

// MODE kEdges / kUpperEdges: item i is edge i of (a = row, b = col), validated against n_a / n_b.
// MODE kCsr: item i is CSR position i, a = perm (b unused); an id outside [0, E) is never kept.
template <int MODE>
__device__ __forceinline__ bool item_keep(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t i, int64_t E,
                                          int64_t n_a, int64_t n_b, uint32_t thr, uint64_t seed, int& bad)
{
    if (i >= E) return false;
    if constexpr (MODE == kCsr) {
        const int32_t id = a[i];
        return id >= 0 && id < E && keep_id(thr, seed, uint32_t(id));
    } else {
        const int32_t r = a[i], c = b[i];
        bad |= !((r >= 0) & (r < n_a) & (c >= 0) & (c < n_b));
        if constexpr (MODE == kUpperEdges) {
            if (!(r < c)) return false;
        }
        return keep_id(thr, seed, uint32_t(i));
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) tile_count(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t E,
                                                     int64_t n_a, int64_t n_b, uint32_t thr, uint64_t seed,
                                                     int32_t* __restrict__ tile_cnt, int32_t* __restrict__ flag)
{
    int bad = 0;
    compact::tile_count([&](int64_t i) { return item_keep<MODE>(a, b, i, E, n_a, n_b, thr, seed, bad); }, tile_cnt);
    if (MODE != kCsr && __any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flag, 1);
}

// The order-stable compaction of tfgx_compact.h:
//   kEdges      : out_a / out_b / out_c [pos] = row, col, edge id
//   kUpperEdges : the same, and the flipped edge with the same id at [half + pos]
//   kCsr        : out_a [pos] = col (b), out_b [pos] = new id of edge perm (a) through the edge-order group table `rank_of`
// `table` (may be null) receives this pass's own group entries.  Nothing is written at or past `cap`.
template <int MODE>
__global__ void __launch_bounds__(kBlock) tile_emit(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t E,
                                                    uint32_t thr, uint64_t seed, const int32_t* __restrict__ tile_off,
                                                    int32_t cap, int32_t half, const int4* __restrict__ rank_of,
                                                    int32_t* __restrict__ out_a, int32_t* __restrict__ out_b,
                                                    int32_t* __restrict__ out_c, int4* __restrict__ table)
{
    const int lane = threadIdx.x & (kWave - 1);
    uint64_t mask[kTileItems];
    int32_t va[kTileItems], vb[kTileItems];
    int unused = 0;
#pragma unroll
    for (int it = 0; it < kTileItems; ++it) {
        const int64_t i = tile_item(it);
        va[it] = 0;
        vb[it] = 0;
        if (i < E) {
            va[it] = a[i];
            vb[it] = b[i];
        }
        // the count pass validated the endpoints; n_a = n_b = INT32_MAX: no range to check here
        mask[it] = __ballot(item_keep<MODE>(a, b, i, E, int64_t(1) << 31, int64_t(1) << 31, thr, seed, unused));
    }
    compact::tile_positions(mask, tile_off, [&](int it, int32_t first, int32_t pos) {
        const int64_t i = tile_item(it);
        if (table != nullptr && lane == 0 && i < E)
            table[i >> 6] = make_int4(int32_t(uint32_t(mask[it])), int32_t(uint32_t(mask[it] >> 32)), first, 0);
        if (((mask[it] >> lane) & 1) && pos < cap) {
            if constexpr (MODE == kCsr) {
                out_a[pos] = vb[it];
                out_b[pos] = group_rank(rank_of, va[it]);      // va = perm[i], inside [0, E): item_keep checked it
            } else {
                out_a[pos] = va[it];
                out_b[pos] = vb[it];
                out_c[pos] = int32_t(i);
                if constexpr (MODE == kUpperEdges) {
                    out_a[half + pos] = vb[it];
                    out_b[half + pos] = va[it];
                    out_c[half + pos] = int32_t(i);
                }
            }
        }
    });
}

// out_row_ptr[r] = kept CSR positions below parent_row_ptr[r]; `total` (device) = all kept positions
__global__ void row_ptr_map(const int32_t* __restrict__ parent_row_ptr, int64_t n_rows, int64_t E,
                            const int4* __restrict__ table, const int32_t* __restrict__ total, int32_t cap,
                            int32_t* __restrict__ out_row_ptr)
{
    int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (; r <= n_rows; r += stride) {
        const int64_t p = parent_row_ptr[r];
        int32_t v = p <= 0 ? 0 : (p >= E ? *total : group_rank(table, p));
        out_row_ptr[r] = v < cap ? v : cap;
    }
}

struct Layout {
    int64_t nt, ng;
    size_t off_tile_cnt, off_tile_off, off_etab, off_ctile_cnt, off_ctile_off, off_ctab, off_temp, temp_bytes, total;
};

// Workspace: [tile_cnt (nt + 1) | tile_off (nt + 1), flag (1) | edge-order group table (ng x 16 B) | CSR tile_cnt (nt + 1) |
// CSR tile_off (nt + 1) | CSR-order group table (ng x 16 B) | scan temp]; the tables and the CSR arrays only with a plan (the
// by-destination and the by-source plan use the CSR part one after the other).  tile_off[nt] (the kept total) and the flag
// are ONE contiguous 8-byte block, fetched with a single device -> host copy.
Layout layout(int64_t E, int with_any_plan)
{
    Layout L;
    L.nt = num_tiles(E);
    L.ng = num_groups(E);
    L.temp_bytes = align256(scan_bytes(L.nt + 1));
    const size_t tiles = align256(sizeof(int32_t) * size_t(L.nt + 2));
    const size_t table = with_any_plan ? align256(sizeof(int4) * size_t(L.ng > 0 ? L.ng : 1)) : 0;
    L.off_tile_cnt = 0;
    L.off_tile_off = tiles;
    L.off_etab = 2 * tiles;
    L.off_ctile_cnt = L.off_etab + table;
    L.off_ctile_off = L.off_ctile_cnt + (with_any_plan ? tiles : 0);
    L.off_ctab = L.off_ctile_off + (with_any_plan ? tiles : 0);
    L.off_temp = L.off_ctab + table;
    L.total = L.off_temp + L.temp_bytes;
    return L;
}

int check_common(const char* fn, const int32_t* row, const int32_t* col, int64_t E, int64_t n_dst, int64_t n_src, float rate,
                 int32_t force_undirected)
{
    if (!(rate >= 0.0f && rate <= 1.0f)) {
        set_error("%s: rate must be in [0, 1], got %g", fn, double(rate));
        return TFGX_ERR_INVALID_ARG;
    }
    if (E < 0 || n_dst < 0 || n_src < 0) {
        set_error("%s: negative size (E = %lld, n_dst = %lld, n_src = %lld)", fn, (long long)E, (long long)n_dst, (long long)n_src);
        return TFGX_ERR_INVALID_ARG;
    }
    if (E >= kMaxSize || n_dst >= kMaxSize || n_src >= kMaxSize) {
        set_error("%s: E, n_dst and n_src must fit int32", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    if (force_undirected != 0 && force_undirected != 1) {
        set_error("%s: force_undirected must be 0 or 1", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    if (force_undirected && n_dst != n_src) {
        set_error("%s: force_undirected needs n_dst == n_src", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    if (E > 0 && (row == nullptr || col == nullptr)) {
        set_error("%s: %s is null", fn, row == nullptr ? "row" : "col");
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

int check_workspace(const char* fn, const void* workspace, size_t workspace_bytes, const Layout& lay)
{
    if (workspace == nullptr) {
        set_error("%s: workspace is null", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    if (!aligned_to(workspace, 16)) {
        set_error("%s: workspace must be 16-byte aligned", fn);
        return TFGX_ERR_INVALID_ARG;
    }
    if (workspace_bytes < lay.total) {
        set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, lay.total);
        return TFGX_ERR_WORKSPACE;
    }
    return TFGX_OK;
}

int check_plan(const char* fn, const char* which, const tfgx_drop_edge_plan* p, int64_t E, int64_t n_out)
{
    if (p == nullptr) return TFGX_OK;
    const char* bad = nullptr;
    if (p->parent_row_ptr == nullptr) bad = "parent_row_ptr";
    else if (p->out_row_ptr == nullptr) bad = "out_row_ptr";
    else if (E > 0 && p->parent_col == nullptr) bad = "parent_col";
    else if (E > 0 && p->parent_perm == nullptr) bad = "parent_perm";
    else if (n_out > 0 && p->out_col == nullptr) bad = "out_col";
    else if (n_out > 0 && p->out_perm == nullptr) bad = "out_perm";
    if (bad != nullptr) {
        set_error("%s: %s->%s is null", fn, which, bad);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

// One derived plan: compaction of the parent's (col, perm) in CSR order, then the row_ptr map.
int derive_plan(const tfgx_drop_edge_plan& p, int64_t n_rows, int64_t E, int64_t n_out, uint32_t thr, uint64_t seed,
                char* ws, const Layout& lay, hipStream_t stream)
{
    if (n_out == 0 || E == 0) {
        TFGX_HIP_CHECK(hipMemsetAsync(p.out_row_ptr, 0, sizeof(int32_t) * size_t(n_rows + 1), stream));
        return TFGX_OK;
    }
    int32_t* tile_cnt = reinterpret_cast<int32_t*>(ws + lay.off_ctile_cnt);
    int32_t* tile_off = reinterpret_cast<int32_t*>(ws + lay.off_ctile_off);
    const int4* etab = reinterpret_cast<const int4*>(ws + lay.off_etab);
    int4* ctab = reinterpret_cast<int4*>(ws + lay.off_ctab);
    const unsigned nt = static_cast<unsigned>(lay.nt);
    TFGX_HIP_CHECK(hipMemsetAsync(tile_cnt + lay.nt, 0, sizeof(int32_t), stream));
    tile_count<kCsr><<<nt, kBlock, 0, stream>>>(p.parent_perm, nullptr, E, 0, 0, thr, seed, tile_cnt, nullptr);
    TFGX_LAUNCH_CHECK("tile_count<csr>");
    size_t tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.off_temp, tb, tile_cnt, tile_off, static_cast<int>(lay.nt + 1),
                                                    stream));
    tile_emit<kCsr><<<nt, kBlock, 0, stream>>>(p.parent_perm, p.parent_col, E, thr, seed, tile_off, int32_t(n_out), 0, etab,
                                               p.out_col, p.out_perm, nullptr, ctab);
    TFGX_LAUNCH_CHECK("tile_emit<csr>");
    row_ptr_map<<<grid_for(n_rows + 1, kBlock), kBlock, 0, stream>>>(p.parent_row_ptr, n_rows, E, ctab, tile_off + lay.nt,
                                                                     int32_t(n_out), p.out_row_ptr);
    TFGX_LAUNCH_CHECK("row_ptr_map");
    return TFGX_OK;
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_dropedge_version(void) { return TFGX_DROPEDGE_ABI_VERSION; }

extern "C" size_t tfgx_drop_edge_workspace_bytes(int64_t E, int64_t n_dst, int64_t n_src, int32_t with_plan, int32_t with_plan_t)
{
    if (E < 0 || n_dst < 0 || n_src < 0 || E >= kMaxSize) return 0;
    return layout(E, with_plan || with_plan_t).total;
}

extern "C" int tfgx_drop_edge_count(const int32_t* row, const int32_t* col, int64_t E, int64_t n_dst, int64_t n_src, float rate,
                                    uint64_t seed, int32_t force_undirected, int64_t* n_out, void* workspace,
                                    size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_common(__func__, row, col, E, n_dst, n_src, rate, force_undirected)) return rc;
    TFGX_REQUIRE(n_out != nullptr, "n_out (host) is null");
    *n_out = 0;
    if (E == 0) return TFGX_OK;
    const Layout lay = layout(E, 0);
    if (int rc = check_workspace(__func__, workspace, workspace_bytes, lay)) return rc;
    char* ws = static_cast<char*>(workspace);
    int32_t* tile_cnt = reinterpret_cast<int32_t*>(ws + lay.off_tile_cnt);
    int32_t* tile_off = reinterpret_cast<int32_t*>(ws + lay.off_tile_off);
    int32_t* flag = tile_off + lay.nt + 1;
    const uint32_t thr = make_drop(rate, seed, 0).thr;
    const unsigned nt = static_cast<unsigned>(lay.nt);

    TFGX_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int32_t), stream));
    TFGX_HIP_CHECK(hipMemsetAsync(tile_cnt + lay.nt, 0, sizeof(int32_t), stream));
    if (force_undirected)
        tile_count<kUpperEdges><<<nt, kBlock, 0, stream>>>(row, col, E, n_dst, n_src, thr, seed, tile_cnt, flag);
    else
        tile_count<kEdges><<<nt, kBlock, 0, stream>>>(row, col, E, n_dst, n_src, thr, seed, tile_cnt, flag);
    TFGX_LAUNCH_CHECK("tile_count");
    size_t tb = lay.temp_bytes;
    TFGX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws + lay.off_temp, tb, tile_cnt, tile_off, static_cast<int>(lay.nt + 1),
                                                    stream));
    int32_t host[2] = {0, 0};      // {kept candidates, bad edge endpoint}
    TFGX_HIP_CHECK(hipMemcpyAsync(host, tile_off + lay.nt, sizeof(host), hipMemcpyDeviceToHost, stream));
    TFGX_HIP_CHECK(hipStreamSynchronize(stream));
    if (host[1]) {
        set_error("tfgx_drop_edge_count: edge endpoint outside [0, %lld) x [0, %lld)", (long long)n_dst, (long long)n_src);
        return TFGX_ERR_INDEX;
    }
    *n_out = force_undirected ? 2 * int64_t(host[0]) : int64_t(host[0]);
    return TFGX_OK;
}

extern "C" int tfgx_drop_edge_emit(const int32_t* row, const int32_t* col, int64_t E, int64_t n_dst, int64_t n_src, float rate,
                                   uint64_t seed, int32_t force_undirected, int64_t n_out, int32_t* out_row, int32_t* out_col,
                                   int32_t* out_edge_id, const tfgx_drop_edge_plan* plan, const tfgx_drop_edge_plan* plan_t,
                                   void* workspace, size_t workspace_bytes, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    if (int rc = check_common(__func__, row, col, E, n_dst, n_src, rate, force_undirected)) return rc;
    // force_undirected: every kept candidate is emitted twice, so up to 2 E edges (a list of upper edges only)
    TFGX_REQUIRE(n_out >= 0 && n_out <= (force_undirected ? 2 * E : E) && (!force_undirected || n_out % 2 == 0),
                 "n_out is not what tfgx_drop_edge_count returns");
    const int with_plan = plan != nullptr || plan_t != nullptr;
    TFGX_REQUIRE(!(with_plan && force_undirected), "plan / plan_t cannot be derived together with force_undirected");
    if (n_out > 0 && (out_row == nullptr || out_col == nullptr || out_edge_id == nullptr)) {
        set_error("%s: %s is null", __func__, out_row == nullptr ? "out_row" : (out_col == nullptr ? "out_col" : "out_edge_id"));
        return TFGX_ERR_INVALID_ARG;
    }
    if (int rc = check_plan(__func__, "plan", plan, E, n_out)) return rc;
    if (int rc = check_plan(__func__, "plan_t", plan_t, E, n_out)) return rc;
    const Layout lay = layout(E, with_plan);
    char* ws = static_cast<char*>(workspace);
    const uint32_t thr = make_drop(rate, seed, 0).thr;
    if (n_out > 0) {
        if (int rc = check_workspace(__func__, workspace, workspace_bytes, lay)) return rc;
        const int32_t* tile_off = reinterpret_cast<const int32_t*>(ws + lay.off_tile_off);
        int4* etab = with_plan ? reinterpret_cast<int4*>(ws + lay.off_etab) : nullptr;
        const unsigned nt = static_cast<unsigned>(lay.nt);
        if (force_undirected)
            tile_emit<kUpperEdges><<<nt, kBlock, 0, stream>>>(row, col, E, thr, seed, tile_off, int32_t(n_out / 2),
                                                              int32_t(n_out / 2), nullptr, out_row, out_col, out_edge_id, etab);
        else
            tile_emit<kEdges><<<nt, kBlock, 0, stream>>>(row, col, E, thr, seed, tile_off, int32_t(n_out), 0, nullptr, out_row,
                                                         out_col, out_edge_id, etab);
        TFGX_LAUNCH_CHECK("tile_emit");
    }
    if (plan != nullptr)
        if (int rc = derive_plan(*plan, n_dst, E, n_out, thr, seed, ws, lay, stream)) return rc;
    if (plan_t != nullptr)
        if (int rc = derive_plan(*plan_t, n_src, E, n_out, thr, seed, ws, lay, stream)) return rc;
    return TFGX_OK;
}
