// One fixed-shape SAGPool level (include/tfgx_pool_static.h, where the layout is written down): static batch in, static batch
// out.  Every launch is sized by capacities the host knows; the live totals (m_live, e_kept) are read from device memory by the
// kernels that need them, never by the host.
//
// Reference: tf_geometric/nn/pool/topk_pool.py:6-87, nn/pool/sag_pool.py:7-45, data/graph.py:276-359.
//
// table  : ONE workgroup of kScanBlock threads, thread t owns a contiguous run of slots; an exclusive scan of k_g (the scan and
//          the runs are tfgx_compact.h's, and so is the tile compaction of the edges below).
// select : one workgroup per slot.  The slot's (descending_bits(score) << 32 | position) keys go to LDS; every node's rank is the
//          number of keys below its own — the keys are distinct, so the ranks are a permutation, ties fall in row order, and
//          the order is that of tfgx_segment_topk's stable radix sort on the same 32 bits.  Each thread holds kSelItems keys in
//          registers and streams the LDS keys past them (one broadcast ds_read_b64 serves kSelItems compares of all 256 lanes:
//          no bank conflict).  O(n_g^2) compares: 10-50-node graphs take one pass of a few dozen reads; the 4096-node cap takes
//          4 passes of 4096 reads.  Behind the slots, two fill sections: the dead pooled rows, the dead parent rows.
// edges  : count (kept edges per tile of kTile; kept edges per pooled row of both parent plans) -> scan (three workgroups: the
//          tiles, the rows of each plan; dead rows in closed form) -> emit edges (order-stable compaction by wave ballot, and the
//          padded tail) -> emit plans (pooled row j = parent row node_index[j] in CSR order).
// No global atomics, no float atomics: every output is a pure function of the inputs.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "tfgx_gather.h"
#include "tfgx_collate_tiles.h"
#include "tfgx_topk_keys.h"
#include "../../include/tfgx_pool_static.h"

namespace tfgx {
namespace {

using namespace compact;
using collate::PlanDev;

constexpr int kMaxGraph = TFGX_STATIC_POOL_MAX_GRAPH_NODES;
constexpr int kSelItems = 4;                           // keys a thread ranks per pass over the LDS keys
constexpr int kFillTile = kBlock * 4;                  // rows per workgroup of the fill sections
constexpr int kRowLanes = 8;                           // lanes that walk one pooled row (graph batches: a few edges per node)
constexpr int kRowsPerBlock = kBlock / kRowLanes;
static_assert(kMaxGraph % (kBlock * kSelItems) == 0, "the cap is a whole number of ranking passes");

// ---- (a) the pooled table ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t kept_of_slot(const int32_t* __restrict__ grp, int32_t j, int32_t k, float ratio, int32_t& flags)
{
    const int32_t n = max(grp[j + 1] - grp[j], 0);
    if (n > kMaxGraph) {
        flags |= TFGX_STATIC_POOL_TOO_LONG;
        return 0;
    }
    return max(topk_node_k(n, k, ratio), 0);
}

__global__ void __launch_bounds__(kScanBlock) pool_table_kernel(const int32_t* __restrict__ grp, const int32_t* __restrict__ parent_counts,
                                                                int32_t B, int32_t k, float ratio, int32_t m_max, int32_t n_cap_out,
                                                                int32_t* __restrict__ prp, int32_t* __restrict__ counts)
{
    __shared__ int32_t s_flags;
    if (threadIdx.x == 0) s_flags = 0;
    const auto [begin, end] = thread_run(B);
    int64_t mine = 0;
    int32_t flags = 0;
    for (int32_t j = begin; j < end; ++j) mine += kept_of_slot(grp, j, k, ratio, flags);
    int64_t total;
    int64_t run = block_exclusive_scan(mine, total);
    for (int32_t j = begin; j < end; ++j) {
        prp[j] = int32_t(min(run, int64_t(m_max)));
        run += kept_of_slot(grp, j, k, ratio, flags);
    }
    if (flags != 0) atomicOr(&s_flags, flags);          // LDS, commutative
    __syncthreads();
    if (threadIdx.x == 0) {
        const int32_t m_live = int32_t(min(total, int64_t(m_max)));
        prp[B] = m_live;
        prp[B + 1] = n_cap_out;
        counts[0] = parent_counts[0];
        counts[1] = m_live;
        counts[2] = 0;
        counts[3] = parent_counts[3] | s_flags | (total > m_max ? TFGX_STATIC_POOL_CLAMPED : 0);
    }
}

// ---- (b) the selection -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) pool_select_kernel(const float* __restrict__ score, const int32_t* __restrict__ grp,
                                                             const int32_t* __restrict__ prp, int32_t B, int32_t n_cap, int32_t sinks,
                                                             int32_t n_cap_out, int32_t out_tiles, int32_t* __restrict__ node_index,
                                                             int32_t* __restrict__ ngi_out, int32_t* __restrict__ node_map)
{
    __shared__ uint64_t keys[kMaxGraph];                // 32 KiB
    const int32_t b = int32_t(blockIdx.x);
    // the live totals, held to the capacities whatever the tables say: no store leaves the outputs
    const int32_t n_live = clampi(grp[B], 0, n_cap - sinks);
    const int32_t m_live = clampi(prp[B], 0, max(n_cap_out - sinks, 0));
    if (b < B) {
        const int32_t r0 = clampi(grp[b], 0, n_live), r1 = clampi(grp[b + 1], r0, n_live);
        const int32_t p0 = clampi(prp[b], 0, m_live), p1 = clampi(prp[b + 1], p0, m_live);
        const int32_t n = r1 - r0, kg = p1 - p0;
        if (n > kMaxGraph) {                            // flagged by the table; keeps no node (workgroup-uniform)
            for (int32_t i = threadIdx.x; i < n; i += kBlock) node_map[r0 + i] = -1;
            return;
        }
        for (int32_t i = threadIdx.x; i < n; i += kBlock)
            keys[i] = (uint64_t(descending_bits(score[r0 + i])) << 32) | uint32_t(i);
        __syncthreads();
        for (int32_t i0 = 0; i0 < n; i0 += kBlock * kSelItems) {
            uint64_t mine[kSelItems];
            int32_t below[kSelItems];
#pragma unroll
            for (int t = 0; t < kSelItems; ++t) {
                const int32_t i = i0 + t * kBlock + int32_t(threadIdx.x);
                mine[t] = i < n ? keys[i] : 0;          // key 0 has nothing below it
                below[t] = 0;
            }
            for (int32_t j = 0; j < n; ++j) {
                const uint64_t kj = keys[j];            // one address for the whole wave: a broadcast read
#pragma unroll
                for (int t = 0; t < kSelItems; ++t) below[t] += kj < mine[t] ? 1 : 0;
            }
#pragma unroll
            for (int t = 0; t < kSelItems; ++t) {
                const int32_t i = i0 + t * kBlock + int32_t(threadIdx.x);
                if (i >= n) continue;
                const bool keep = below[t] < kg;        // rank = below[t]; kg <= m_live - p0, so p0 + rank < m_live
                const int32_t pos = p0 + below[t];
                if (keep) {
                    node_index[pos] = r0 + i;
                    ngi_out[pos] = b;
                }
                node_map[r0 + i] = keep ? pos : -1;
            }
        }
    } else if (b < B + out_tiles) {                     // the dead pooled rows
#pragma unroll
        for (int it = 0; it < kFillTile / kBlock; ++it) {
            const int64_t j = int64_t(b - B) * kFillTile + it * kBlock + threadIdx.x;
            if (j >= m_live && j < n_cap_out) {
                node_index[j] = -1;
                ngi_out[j] = B;
            }
        }
    } else {                                            // the dead parent rows
#pragma unroll
        for (int it = 0; it < kFillTile / kBlock; ++it) {
            const int64_t i = int64_t(b - B - out_tiles) * kFillTile + it * kBlock + threadIdx.x;
            if (i >= n_live && i < n_cap) node_map[i] = -1;
        }
    }
}

// ---- (c) pooled edges and plans ------------------------------------------------------------------------------------------------
struct EdgeParams {
    const int32_t* row;
    const int32_t* col;
    const float* w;
    const int32_t* egi;
    const int32_t* node_map;
    const int32_t* node_index;
    const int32_t* prp;
    int32_t n_cap, e_cap, B, sinks, sink_degree, n_cap_out;
    int32_t m_rows;                    // n_cap_out - sinks: the rows that can be live
    int32_t nt;                        // edge tiles
    int32_t* out_row;
    int32_t* out_col;
    int32_t* out_edge_id;
    int32_t* out_egi;
    float* out_w;
    PlanDev plan[2];                   // ds_* = the parent's plan, out_* = the pooled one
    int32_t* counts;
    int32_t* tile_cnt;                 // [nt]
    int32_t* tile_off;                 // [nt + 1]
    int32_t* row_cnt;                  // [2, m_rows]
    int32_t* rank;                     // [e_cap]: parent edge -> pooled edge, for the kept ones
};

__device__ __forceinline__ int32_t live_pooled_rows(const EdgeParams& p) { return clampi(p.prp[p.B], 0, p.m_rows); }

// new endpoints of parent edge e, or -1: an endpoint is compared with the rows before it is an index
__device__ __forceinline__ bool kept_edge(const EdgeParams& p, int64_t e, int32_t& nr, int32_t& nc)
{
    nr = nc = -1;
    if (e >= p.e_cap) return false;
    const int32_t r = p.row[e], c = p.col[e];
    if (r < 0 || r >= p.n_cap || c < 0 || c >= p.n_cap) return false;
    nr = p.node_map[r];
    nc = p.node_map[c];
    return nr >= 0 && nc >= 0 && nr < p.m_rows && nc < p.m_rows;
}

// the kept part [s, t) of parent row node_index[j] of plan k: both ends held to the edge capacity
__device__ __forceinline__ void parent_span(const EdgeParams& p, int k, int32_t j, int32_t m_live, int32_t& s, int32_t& t)
{
    s = t = 0;
    if (j >= m_live) return;
    const int32_t o = p.node_index[j];
    if (o < 0 || o >= p.n_cap) return;
    s = clampi(p.plan[k].ds_row_ptr[o], 0, p.e_cap);
    t = clampi(p.plan[k].ds_row_ptr[o + 1], s, p.e_cap);
}

__device__ __forceinline__ int32_t mapped_source(const EdgeParams& p, int k, int32_t pos)
{
    const int32_t c = p.plan[k].ds_col[pos];
    if (c < 0 || c >= p.n_cap) return -1;
    const int32_t nc = p.node_map[c];
    return nc < p.m_rows ? nc : -1;
}

// sections: [0, nt) kept edges per tile; behind them kept edges per pooled row, kRowLanes lanes to a row, both plans
__global__ void __launch_bounds__(kBlock) pool_count_kernel(const EdgeParams p)
{
    if (int32_t(blockIdx.x) < p.nt) {
        tile_count(
            [&](int64_t e) {
                int32_t nr, nc;
                return kept_edge(p, e, nr, nc);
            },
            p.tile_cnt);
        return;
    }
    const int32_t m_live = live_pooled_rows(p);
    const int lig = threadIdx.x % kRowLanes;
    const int64_t j64 = (int64_t(blockIdx.x) - p.nt) * kRowsPerBlock + threadIdx.x / kRowLanes;
    if (j64 >= p.m_rows) return;
    const int32_t j = int32_t(j64);
    for (int k = 0; k < 2; ++k) {
        int32_t s, t, c = 0;
        parent_span(p, k, j, m_live, s, t);
        for (int32_t b = s; b < t; b += kRowLanes) {
            const int32_t pos = b + lig;
            c += __popcll(group_bits<kRowLanes>(pos < t && mapped_source(p, k, pos) >= 0));
        }
        if (lig == 0) p.row_cnt[int64_t(k) * p.m_rows + j] = c;
    }
}

// workgroup 0: tile_off = exclusive sums of tile_cnt, counts[2] = e_kept.  Workgroups 1, 2: the row_ptr of plan 0, 1 — the
// exclusive sums of row_cnt over the rows that can be live (a dead one counts 0), then the sink rows in closed form.
__global__ void __launch_bounds__(kScanBlock) pool_scan_kernel(const EdgeParams p)
{
    const bool tiles = blockIdx.x == 0;
    const int32_t n = tiles ? p.nt : p.m_rows;
    const int32_t* in = tiles ? p.tile_cnt : p.row_cnt + int64_t(blockIdx.x - 1) * p.m_rows;
    int32_t* out = tiles ? p.tile_off : p.plan[blockIdx.x - 1].out_row_ptr;
    const auto [begin, end] = thread_run(n);
    int64_t mine = 0;
    for (int32_t j = begin; j < end; ++j) mine += in[j];
    int64_t total;
    int64_t run = block_exclusive_scan(mine, total);
    for (int32_t j = begin; j < end; ++j) {
        out[j] = int32_t(min(run, int64_t(p.e_cap)));
        run += in[j];
    }
    const int32_t e_kept = int32_t(min(total, int64_t(p.e_cap)));
    if (tiles) {
        if (threadIdx.x == 0) {
            out[n] = e_kept;
            p.counts[2] = e_kept;
        }
        return;
    }
    // rows m_rows + t, t in [0, sinks]: sink t holds the padded edges [t, t + 1) * sink_degree of the tail
    for (int32_t t = threadIdx.x; t <= p.sinks; t += kScanBlock)
        out[p.m_rows + t] = e_kept + int32_t(min(int64_t(p.e_cap - e_kept), int64_t(t) * p.sink_degree));
}

// The order-stable compaction of tfgx_compact.h over tile blockIdx.x of the parent edges, then the part of the padded tail that
// lies in the output positions of the same numbers, [blockIdx.x, blockIdx.x + 1) * kTile.
__global__ void __launch_bounds__(kBlock) pool_emit_edges_kernel(const EdgeParams p)
{
    const int32_t e_kept = clampi(p.tile_off[p.nt], 0, p.e_cap);
    uint64_t mask[kTileItems];
    int32_t nr[kTileItems], nc[kTileItems];
    bool keep[kTileItems];
#pragma unroll
    for (int it = 0; it < kTileItems; ++it) {
        keep[it] = kept_edge(p, tile_item(it), nr[it], nc[it]);
        mask[it] = __ballot(keep[it]);
    }
    tile_positions(mask, p.tile_off, [&](int it, int32_t, int32_t pos) {
        if (keep[it] && pos >= 0 && pos < e_kept) {
            const int64_t e = tile_item(it);
            p.out_row[pos] = nr[it];
            p.out_col[pos] = nc[it];
            p.out_edge_id[pos] = int32_t(e);
            p.out_egi[pos] = p.egi[e];
            if (p.out_w != nullptr) p.out_w[pos] = p.w != nullptr ? p.w[e] : 1.0f;
            p.rank[e] = pos;
        }
    });
#pragma unroll
    for (int it = 0; it < kTileItems; ++it) {
        const int64_t q64 = tile_item(it);
        if (q64 < e_kept || q64 >= p.e_cap) continue;
        const int32_t q = int32_t(q64);
        const int32_t v = p.m_rows + (q - e_kept) / p.sink_degree;      // < n_cap_out: sinks * sink_degree >= e_cap
        p.out_row[q] = v;
        p.out_col[q] = v;
        p.out_edge_id[q] = -1;
        p.out_egi[q] = p.B;
        if (p.out_w != nullptr) p.out_w[q] = 1.0f;
        for (int k = 0; k < 2; ++k) {                                   // its own CSR position in both plans
            p.plan[k].out_col[q] = v;
            p.plan[k].out_perm[q] = q;
        }
    }
}

// pooled row j = the kept part of parent row node_index[j], in CSR order, for both plans
__global__ void __launch_bounds__(kBlock) pool_emit_plans_kernel(const EdgeParams p)
{
    const int32_t m_live = live_pooled_rows(p);
    const int32_t e_kept = clampi(p.tile_off[p.nt], 0, p.e_cap);
    const int lig = threadIdx.x % kRowLanes;
    const uint64_t below = (uint64_t(1) << lig) - 1;
    const int64_t j64 = int64_t(blockIdx.x) * kRowsPerBlock + threadIdx.x / kRowLanes;
    if (j64 >= m_live) return;
    const int32_t j = int32_t(j64);
    for (int k = 0; k < 2; ++k) {
        int32_t s, t;
        parent_span(p, k, j, m_live, s, t);
        int32_t pos = p.plan[k].out_row_ptr[j];
        for (int32_t b = s; b < t; b += kRowLanes) {
            const int32_t at = b + lig;
            const int32_t nc = at < t ? mapped_source(p, k, at) : -1;
            const uint64_t bits = group_bits<kRowLanes>(nc >= 0);
            if (nc >= 0) {
                const int32_t q = pos + __popcll(bits & below);
                const int32_t pe = p.plan[k].ds_perm[at];
                if (q >= 0 && q < e_kept) {
                    p.plan[k].out_col[q] = nc;
                    p.plan[k].out_perm[q] = (pe >= 0 && pe < p.e_cap) ? p.rank[pe] : -1;
                }
            }
            pos += __popcll(bits);
        }
    }
}

Workspace<4> edges_workspace(int64_t n_cap_out, int64_t e_cap)
{
    const size_t nt = size_t((e_cap + kTile - 1) / kTile);
    return Workspace<4>{{4 * (nt + 1), 4 * (nt + 1), 8 * size_t(n_cap_out + 1), 4 * size_t(e_cap > 0 ? e_cap : 1)}};
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_static_pool_version(void) { return TFGX_STATIC_POOL_ABI_VERSION; }

extern "C" int tfgx_static_pool_table(const int32_t* graph_row_ptr, const int32_t* parent_counts, int64_t B, int32_t k, float ratio,
                                      int64_t m_max, int64_t n_cap_out, int32_t* pooled_row_ptr, int32_t* counts,
                                      tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const char* fn = "tfgx_static_pool_table";
    const NamedSize sizes[] = {{"B", B}, {"m_max", m_max}, {"n_cap_out", n_cap_out}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (B > TFGX_STATIC_POOL_MAX_SLOTS) {
        set_error("%s: B = %lld is more than the %d slots one workgroup scans", fn, (long long)B, TFGX_STATIC_POOL_MAX_SLOTS);
        return TFGX_ERR_INVALID_ARG;
    }
    if (n_cap_out < m_max) {
        set_error("%s: n_cap_out = %lld is smaller than m_max = %lld", fn, (long long)n_cap_out, (long long)m_max);
        return TFGX_ERR_INVALID_ARG;
    }
    if (k < 0 && !(ratio >= 0.0f)) {
        set_error("%s: ratio = %g must be at least 0 when k is negative (k = %d)", fn, double(ratio), int(k));
        return TFGX_ERR_INVALID_ARG;
    }
    if (B == 0 && pooled_row_ptr == nullptr && counts == nullptr) return TFGX_OK;
    if (graph_row_ptr == nullptr) return null_arg(fn, "graph_row_ptr");
    if (parent_counts == nullptr) return null_arg(fn, "parent_counts");
    if (pooled_row_ptr == nullptr) return null_arg(fn, "pooled_row_ptr");
    if (counts == nullptr) return null_arg(fn, "counts");
    pool_table_kernel<<<1, kScanBlock, 0, as_stream(stream_)>>>(graph_row_ptr, parent_counts, int32_t(B), k, ratio, int32_t(m_max),
                                                                int32_t(n_cap_out), pooled_row_ptr, counts);
    TFGX_LAUNCH_CHECK("pool_table_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_static_pool_select(const float* score, const int32_t* graph_row_ptr, const int32_t* pooled_row_ptr, int64_t B,
                                       int64_t n_cap, int64_t sinks, int64_t n_cap_out, int32_t* node_index,
                                       int32_t* node_graph_index, int32_t* node_map, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    const char* fn = "tfgx_static_pool_select";
    const NamedSize sizes[] = {{"B", B}, {"n_cap", n_cap}, {"sinks", sinks}, {"n_cap_out", n_cap_out}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (B > TFGX_STATIC_POOL_MAX_SLOTS) {
        set_error("%s: B = %lld is more than the %d slots of a pooled table", fn, (long long)B, TFGX_STATIC_POOL_MAX_SLOTS);
        return TFGX_ERR_INVALID_ARG;
    }
    if (int rc = check_sinks_within(fn, sinks, "n_cap", n_cap)) return rc;
    if (n_cap == 0 && n_cap_out == 0) return TFGX_OK;
    if (graph_row_ptr == nullptr) return null_arg(fn, "graph_row_ptr");
    if (pooled_row_ptr == nullptr) return null_arg(fn, "pooled_row_ptr");
    if (n_cap > 0 && B > 0 && score == nullptr) return null_arg(fn, "score");
    if (n_cap_out > 0 && node_index == nullptr) return null_arg(fn, "node_index");
    if (n_cap_out > 0 && node_graph_index == nullptr) return null_arg(fn, "node_graph_index");
    if (n_cap > 0 && node_map == nullptr) return null_arg(fn, "node_map");
    const int64_t out_tiles = (n_cap_out + kFillTile - 1) / kFillTile, map_tiles = (n_cap + kFillTile - 1) / kFillTile;
    const int64_t grid = B + out_tiles + map_tiles;       // each term is below 2^31 / 1024 or 2^20
    pool_select_kernel<<<static_cast<unsigned>(grid), kBlock, 0, as_stream(stream_)>>>(
        score, graph_row_ptr, pooled_row_ptr, int32_t(B), int32_t(n_cap), int32_t(sinks), int32_t(n_cap_out), int32_t(out_tiles),
        node_index, node_graph_index, node_map);
    TFGX_LAUNCH_CHECK("pool_select_kernel");
    return TFGX_OK;
}

extern "C" size_t tfgx_static_pool_edges_workspace_bytes(int64_t n_cap_out, int64_t e_cap)
{
    if (n_cap_out < 0 || e_cap < 0 || n_cap_out >= kMaxSize || e_cap >= kMaxSize) return 0;
    return edges_workspace(n_cap_out, e_cap).bytes();
}

extern "C" int tfgx_static_pool_edges(const tfgx_static_pool_args* a, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    const char* fn = "tfgx_static_pool_edges";
    if (a == nullptr) return null_arg(fn, "args");
    const NamedSize sizes[] = {{"n_cap", a->n_cap}, {"e_cap", a->e_cap}, {"B", a->B}, {"sinks", a->sinks},
                               {"sink_degree", a->sink_degree}, {"n_cap_out", a->n_cap_out}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (int rc = check_sink_degree(fn, a->sink_degree)) return rc;
    if (int rc = check_sinks_within(fn, a->sinks, "n_cap_out", a->n_cap_out)) return rc;
    if (int rc = check_sinks_within(fn, a->sinks, "n_cap", a->n_cap)) return rc;
    if (int rc = check_sink_tail(fn, a->sinks, a->sink_degree, a->e_cap)) return rc;
    // no rows and no edges, and nowhere to put the offsets of an empty batch: nothing exists to be written
    if (a->n_cap_out == 0 && a->e_cap == 0 && a->plan == nullptr && a->plan_t == nullptr && a->counts == nullptr) return TFGX_OK;
    const tfgx_collate_plan* plans[2] = {a->plan, a->plan_t};
    const char* const which[2] = {"plan", "plan_t"};
    for (int k = 0; k < 2; ++k) {                       // both plans are derived: a null one is refused
        if (plans[k] == nullptr) return null_arg(fn, which[k]);
        if (int rc = collate::check_plan(fn, which[k], plans[k], a->e_cap, a->e_cap)) return rc;
    }
    const char* bad = nullptr;
    if (a->counts == nullptr) bad = "counts";
    else if (a->pooled_row_ptr == nullptr) bad = "pooled_row_ptr";
    else if (a->workspace == nullptr) bad = "workspace";
    else if (a->n_cap > 0 && a->node_map == nullptr) bad = "node_map";
    else if (a->n_cap_out > 0 && a->node_index == nullptr) bad = "node_index";
    else if (a->e_cap > 0 && a->row == nullptr) bad = "row";
    else if (a->e_cap > 0 && a->col == nullptr) bad = "col";
    else if (a->e_cap > 0 && a->edge_graph_index == nullptr) bad = "edge_graph_index";
    else if (a->e_cap > 0 && a->out_row == nullptr) bad = "out_row";
    else if (a->e_cap > 0 && a->out_col == nullptr) bad = "out_col";
    else if (a->e_cap > 0 && a->out_edge_id == nullptr) bad = "out_edge_id";
    else if (a->e_cap > 0 && a->out_edge_graph_index == nullptr) bad = "out_edge_graph_index";
    if (bad != nullptr) return null_arg(fn, bad);
    const Workspace<4> ws = edges_workspace(a->n_cap_out, a->e_cap);
    if (a->workspace_bytes < ws.bytes()) {
        set_error("%s: workspace_bytes = %zu is smaller than the %zu bytes tfgx_static_pool_edges_workspace_bytes asks for", fn,
                  a->workspace_bytes, ws.bytes());
        return TFGX_ERR_WORKSPACE;
    }

    EdgeParams p = {};
    p.row = a->row, p.col = a->col, p.w = a->w, p.egi = a->edge_graph_index;
    p.node_map = a->node_map, p.node_index = a->node_index, p.prp = a->pooled_row_ptr;
    p.n_cap = int32_t(a->n_cap), p.e_cap = int32_t(a->e_cap), p.B = int32_t(a->B), p.sinks = int32_t(a->sinks);
    p.sink_degree = int32_t(a->sink_degree), p.n_cap_out = int32_t(a->n_cap_out);
    p.m_rows = int32_t(a->n_cap_out - a->sinks);
    p.nt = int32_t((a->e_cap + kTile - 1) / kTile);
    p.out_row = a->out_row, p.out_col = a->out_col, p.out_edge_id = a->out_edge_id, p.out_egi = a->out_edge_graph_index;
    p.out_w = a->out_w;
    for (int k = 0; k < 2; ++k) p.plan[k] = collate::plan_dev(plans[k]);
    p.counts = a->counts;
    p.tile_cnt = ws.at<int32_t>(a->workspace, 0);
    p.tile_off = ws.at<int32_t>(a->workspace, 1);
    p.row_cnt = ws.at<int32_t>(a->workspace, 2);
    p.rank = ws.at<int32_t>(a->workspace, 3);

    const int64_t row_blocks = (int64_t(p.m_rows) + kRowsPerBlock - 1) / kRowsPerBlock;
    if (p.nt + row_blocks > 0) {
        pool_count_kernel<<<static_cast<unsigned>(p.nt + row_blocks), kBlock, 0, stream>>>(p);
        TFGX_LAUNCH_CHECK("pool_count_kernel");
    }
    pool_scan_kernel<<<3, kScanBlock, 0, stream>>>(p);
    TFGX_LAUNCH_CHECK("pool_scan_kernel");
    if (p.nt > 0) {
        pool_emit_edges_kernel<<<static_cast<unsigned>(p.nt), kBlock, 0, stream>>>(p);
        TFGX_LAUNCH_CHECK("pool_emit_edges_kernel");
    }
    if (row_blocks > 0 && p.nt > 0) {
        pool_emit_plans_kernel<<<static_cast<unsigned>(row_blocks), kBlock, 0, stream>>>(p);
        TFGX_LAUNCH_CHECK("pool_emit_plans_kernel");
    }
    return TFGX_OK;
}

extern "C" int tfgx_static_pool_gather_scale_rows_f32(const float* x, int64_t ldx, int64_t n, const int32_t* idx, const float* s,
                                                      int64_t M, int64_t F, float* out, int64_t ldo, tfgx_stream_t stream)
{
    TFGX_RANGE();
    const char* fn = "tfgx_static_pool_gather_scale_rows_f32";
    const NamedSize sizes[] = {{"n", n}, {"M", M}, {"F", F}};
    if (int rc = check_sizes(fn, sizes)) return rc;
    if (ldx < F) return bad_arg(fn, "ldx is smaller than F", ldx);
    if (ldo < F) return bad_arg(fn, "ldo is smaller than F", ldo);
    if (M == 0 || F == 0) return TFGX_OK;
    if (n == 0) return bad_arg(fn, "n must be at least 1 (the clamped load needs a row)", n);
    if (x == nullptr) return null_arg(fn, "x");
    if (idx == nullptr) return null_arg(fn, "idx");
    if (out == nullptr) return null_arg(fn, "out");
    const bool vec = ldx % 4 == 0 && ldo % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 16);
    const int64_t F4 = vec ? F / 4 : 0;
    gather_scale_rows<true><<<grid_for(M * (F4 + F - 4 * F4), kBlock), kBlock, 0, as_stream(stream)>>>(x, ldx, n, idx, s, M, F, F4,
                                                                                                       out, ldo);
    TFGX_LAUNCH_CHECK("gather_scale_rows<clamped>");
    return TFGX_OK;
}
