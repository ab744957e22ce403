// Fixed-shape minibatch assembly (include/tfgx_collate_static.h): the table of a batch from device-resident graph ids in one
// launch, the batch at its capacities in a second one.  Every size a launch needs is a capacity the host knows, the live totals
// are read from the table on the device, nothing is read back.
//
// Reference: tf_geometric/data/graph.py:463-560 (BatchGraph.from_graphs), demo/demo_mean_pool.py (a batch per step).
//
// table  : ONE workgroup of kScanBlock threads; thread t owns a contiguous run of slots (tfgx_compact.h: thread_run).  Two
//          exclusive scans of (nodes, edges) pairs in int64 (tfgx_compact.h: block_exclusive_scan): over the IN-RANGE slots,
//          which decides who is live (both cumulated totals within the capacities), then over the LIVE slots, which gives the
//          output offsets.  The live count and the flags are integer LDS atomics (add / or: commutative).
// collate: the sections of tfgx_collate_tiles.h at STATIC = true, and behind them a graph section that copies out_node_ptr into
//          graph_row_ptr and closes it with n_cap.  No atomics.
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "tfgx_compact.h"
#include "tfgx_collate_tiles.h"
#include "../../include/tfgx_collate_static.h"

namespace tfgx {
namespace {

using namespace collate;

using compact::kScanBlock;
static_assert(int64_t(TFGX_STATIC_BATCH_MAX_SLOTS) >= 65535, "the scan covers at least 65 535 slots");

struct Pair {
    int64_t n, e;
};

__device__ __forceinline__ Pair operator+(Pair a, Pair b) { return Pair{a.n + b.n, a.e + b.e}; }
__device__ __forceinline__ Pair operator-(Pair a, Pair b) { return Pair{a.n - b.n, a.e - b.e}; }
__device__ __forceinline__ Pair shfl_up(Pair v, int off) { return Pair{compact::shfl_up(v.n, off), compact::shfl_up(v.e, off)}; }

__global__ void __launch_bounds__(kScanBlock) collate_static_table_kernel(
    const int32_t* __restrict__ ids, int32_t B, const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ edge_ptr,
    int32_t G, int64_t max_nodes, int64_t max_edges, int32_t* __restrict__ table, uint8_t* __restrict__ live_mask,
    int32_t* __restrict__ counts)
{
    __shared__ int32_t s_live, s_flags;
    if (threadIdx.x == 0) {
        s_live = 0;
        s_flags = 0;
    }
    const auto [begin, end] = compact::thread_run(B);
    // 1. the in-range slots: an id is compared before it is used as an index
    Pair mine{0, 0};
    int32_t flags = 0;
    for (int32_t j = begin; j < end; ++j) {
        const int32_t id = ids[j];
        if (id >= 0 && id < G) mine = mine + Pair{node_ptr[id + 1] - node_ptr[id], edge_ptr[id + 1] - edge_ptr[id]};
        else if (id != TFGX_STATIC_BATCH_DEAD) flags |= TFGX_STATIC_BATCH_BAD_ID;
    }
    Pair total;
    const Pair before = compact::block_exclusive_scan(mine, total);
    // 2. who is live: both cumulated totals through the slot within the capacities
    Pair live{0, 0}, run = before;
    int32_t n_live_slots = 0;
    for (int32_t j = begin; j < end; ++j) {
        const int32_t id = ids[j];
        if (id < 0 || id >= G) continue;
        const Pair size{node_ptr[id + 1] - node_ptr[id], edge_ptr[id + 1] - edge_ptr[id]};
        run = run + size;
        if (run.n <= max_nodes && run.e <= max_edges) {
            live = live + size;
            ++n_live_slots;
        } else {
            flags |= TFGX_STATIC_BATCH_OVERFLOW;
        }
    }
    const Pair out0 = compact::block_exclusive_scan(live, total);      // total: n_live, e_live (within the capacities: int32)
    // 3. the table
    const int64_t stride = int64_t(B) + 1;
    Pair out = out0;
    run = before;
    for (int32_t j = begin; j < end; ++j) {
        const int32_t id = ids[j];
        bool is_live = false;
        Pair size{0, 0};
        if (id >= 0 && id < G) {
            size = Pair{node_ptr[id + 1] - node_ptr[id], edge_ptr[id + 1] - edge_ptr[id]};
            run = run + size;
            is_live = run.n <= max_nodes && run.e <= max_edges;
        }
        table[j] = is_live ? node_ptr[id] : 0;
        table[stride + j] = int32_t(out.n);
        table[2 * stride + j] = is_live ? edge_ptr[id] : 0;
        table[3 * stride + j] = int32_t(out.e);
        live_mask[j] = is_live ? 1 : 0;
        if (is_live) out = out + size;
    }
    if (n_live_slots != 0) atomicAdd(&s_live, n_live_slots);
    if (flags != 0) atomicOr(&s_flags, flags);
    __syncthreads();
    if (threadIdx.x == 0) {
        table[B] = 0;
        table[stride + B] = int32_t(total.n);
        table[2 * stride + B] = 0;
        table[3 * stride + B] = int32_t(total.e);
        counts[0] = s_live;
        counts[1] = int32_t(total.n);
        counts[2] = int32_t(total.e);
        counts[3] = s_flags;
    }
}

// graph_row_ptr [B + 2]: the output offsets of the B slots and of the dead graph B, closed with n_cap
__device__ __forceinline__ void graph_tile(const Params& p, int32_t tile)
{
    const int32_t n_live = live_nodes(p);
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int64_t i = int64_t(tile) * kTile + it * kBlock + threadIdx.x;
        if (i > int64_t(p.B) + 1) break;
        p.graph_row_ptr[i] = i <= p.B ? min(p.out_node_ptr[i], n_live) : p.n_out;
    }
}

template <bool VEC4>
__global__ void __launch_bounds__(kBlock) collate_static_kernel(const Params p)
{
    __shared__ int32_t lds[kLdsOffsets];
    const int64_t b = blockIdx.x;
    if (b < p.x_tiles) feature_tile<VEC4, true>(p, b, lds);
    else if (b < p.x_tiles + p.node_tiles) node_tile<true>(p, int32_t(b - p.x_tiles), lds);
    else if (b < p.x_tiles + p.node_tiles + p.edge_tiles) edge_tile<true>(p, int32_t(b - p.x_tiles - p.node_tiles), lds);
    else graph_tile(p, int32_t(b - p.x_tiles - p.node_tiles - p.edge_tiles));
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_static_batch_version(void) { return TFGX_STATIC_BATCH_ABI_VERSION; }

extern "C" int tfgx_static_batch_table(const int32_t* ids, int64_t B, const int32_t* node_ptr, const int32_t* edge_ptr, int64_t G,
                                       int64_t max_nodes, int64_t max_edges, int32_t* table, uint8_t* live_mask, int32_t* counts,
                                       tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    const NamedSize sizes[] = {{"B", B}, {"G", G}, {"max_nodes", max_nodes}, {"max_edges", max_edges}};
    if (int rc = check_sizes("tfgx_static_batch_table", sizes)) return rc;
    if (B > TFGX_STATIC_BATCH_MAX_SLOTS) {
        set_error("tfgx_static_batch_table: B = %lld is more than the %d slots one workgroup scans", (long long)B,
                  TFGX_STATIC_BATCH_MAX_SLOTS);
        return TFGX_ERR_INVALID_ARG;
    }
    if (B == 0 && table == nullptr && counts == nullptr) return TFGX_OK;
    const char* bad = nullptr;
    if (B > 0 && ids == nullptr) bad = "ids";
    else if (B > 0 && node_ptr == nullptr) bad = "node_ptr";
    else if (B > 0 && edge_ptr == nullptr) bad = "edge_ptr";
    else if (table == nullptr) bad = "table";
    else if (B > 0 && live_mask == nullptr) bad = "live_mask";
    else if (counts == nullptr) bad = "counts";
    if (bad != nullptr) {
        set_error("tfgx_static_batch_table: %s is null", bad);
        return TFGX_ERR_INVALID_ARG;
    }
    collate_static_table_kernel<<<1, kScanBlock, 0, stream>>>(ids, int32_t(B), node_ptr, edge_ptr, int32_t(G), max_nodes, max_edges,
                                                              table, live_mask, counts);
    TFGX_LAUNCH_CHECK("collate_static_table_kernel");
    return TFGX_OK;
}

extern "C" int tfgx_static_batch(const tfgx_static_batch_args* a, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    TFGX_REQUIRE(a != nullptr, "args is null");
    const NamedSize sizes[] = {{"ds_ldx", a->ds_ldx}, {"F", a->F}, {"ds_n", a->ds_n}, {"ds_e", a->ds_e}, {"B", a->B},
                               {"n_cap", a->n_cap}, {"e_cap", a->e_cap}, {"sinks", a->sinks}, {"sink_degree", a->sink_degree},
                               {"out_ldx", a->out_ldx}};
    if (int rc = check_sizes("tfgx_static_batch", sizes)) return rc;
    if (int rc = check_sink_degree("tfgx_static_batch", a->sink_degree)) return rc;
    if (int rc = check_sinks_within("tfgx_static_batch", a->sinks, "n_cap", a->n_cap)) return rc;
    if (int rc = check_sink_tail("tfgx_static_batch", a->sinks, a->sink_degree, a->e_cap)) return rc;
    const bool has_x = a->n_cap > 0 && a->F > 0;
    if (has_x && a->ds_ldx < a->F) {
        set_error("tfgx_static_batch: ds_ldx = %lld is smaller than F = %lld", (long long)a->ds_ldx, (long long)a->F);
        return TFGX_ERR_INVALID_ARG;
    }
    if (has_x && a->out_ldx < a->F) {
        set_error("tfgx_static_batch: out_ldx = %lld is smaller than F = %lld", (long long)a->out_ldx, (long long)a->F);
        return TFGX_ERR_INVALID_ARG;
    }
    // no rows and no edges, and nowhere to put the offsets of an empty batch: nothing exists to be written
    if (a->n_cap == 0 && a->e_cap == 0 && a->plan == nullptr && a->plan_t == nullptr && a->graph_row_ptr == nullptr) return TFGX_OK;
    const char* bad = nullptr;
    if (a->table == nullptr) bad = "table";
    else if (a->plan == nullptr) bad = "plan";
    else if (a->plan_t == nullptr) bad = "plan_t";
    else if (a->graph_row_ptr == nullptr) bad = "graph_row_ptr";
    else if (has_x && a->ds_n > 0 && a->ds_x == nullptr) bad = "ds_x";
    else if (has_x && a->out_x == nullptr) bad = "out_x";
    else if (a->n_cap > 0 && a->out_node_graph_index == nullptr) bad = "out_node_graph_index";
    else if (a->e_cap > 0 && a->ds_e > 0 && a->ds_row == nullptr) bad = "ds_row";
    else if (a->e_cap > 0 && a->ds_e > 0 && a->ds_col == nullptr) bad = "ds_col";
    else if (a->e_cap > 0 && a->out_row == nullptr) bad = "out_row";
    else if (a->e_cap > 0 && a->out_col == nullptr) bad = "out_col";
    else if (a->e_cap > 0 && a->out_edge_graph_index == nullptr) bad = "out_edge_graph_index";
    if (bad != nullptr) {
        set_error("tfgx_static_batch: %s is null", bad);
        return TFGX_ERR_INVALID_ARG;
    }
    if (int rc = check_plan("tfgx_static_batch", "plan", a->plan, a->ds_e, a->e_cap)) return rc;
    if (int rc = check_plan("tfgx_static_batch", "plan_t", a->plan_t, a->ds_e, a->e_cap)) return rc;

    Params p = {};
    p.ds_x = a->ds_x;
    p.ds_ldx = a->ds_ldx;
    p.F = int32_t(a->F);
    p.ds_row = a->ds_row;
    p.ds_col = a->ds_col;
    p.ds_w = a->ds_w;
    const int64_t stride = a->B + 1;
    p.src_node_begin = a->table;
    p.out_node_ptr = a->table + stride;
    p.src_edge_begin = a->table + 2 * stride;
    p.out_edge_ptr = a->table + 3 * stride;
    p.B = int32_t(a->B);
    p.n_out = int32_t(a->n_cap);
    p.e_out = int32_t(a->e_cap);
    p.sinks = int32_t(a->sinks);
    p.sink_degree = int32_t(a->sink_degree);
    p.out_x = a->out_x;
    p.out_ldx = a->out_ldx;
    p.out_ngi = a->out_node_graph_index;
    p.out_row = a->out_row;
    p.out_col = a->out_col;
    p.out_egi = a->out_edge_graph_index;
    p.out_w = a->out_w;
    p.plan[0] = plan_dev(a->plan);
    p.plan[1] = plan_dev(a->plan_t);
    p.graph_row_ptr = a->graph_row_ptr;
    p.node_items = int32_t(a->n_cap + 1);

    const bool vec4 = has_x && a->F % 4 == 0 && a->ds_ldx % 4 == 0 && a->out_ldx % 4 == 0 && aligned_to(a->ds_x, 16) &&
                      aligned_to(a->out_x, 16);
    const int64_t x_items = has_x ? a->n_cap * (vec4 ? a->F / 4 : a->F) : 0;
    const int64_t x_per_tile = vec4 ? kBlock : kTile;              // a tile is kTile floats either way
    p.x_tiles = (x_items + x_per_tile - 1) / x_per_tile;
    p.node_tiles = int32_t((int64_t(p.node_items) + kTile - 1) / kTile);
    p.edge_tiles = int32_t((a->e_cap + kTile - 1) / kTile);
    const int64_t graph_tiles = (a->B + 2 + kTile - 1) / kTile;
    const int64_t grid = p.x_tiles + p.node_tiles + p.edge_tiles + graph_tiles;
    if (grid >= kMaxSize) {
        set_error("tfgx_static_batch: n_cap * F = %lld elements need more workgroups than one launch has",
                  (long long)(a->n_cap * a->F));
        return TFGX_ERR_INVALID_ARG;
    }
    if (vec4) collate_static_kernel<true><<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(p);
    else collate_static_kernel<false><<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(p);
    TFGX_LAUNCH_CHECK("collate_static_kernel");
    return TFGX_OK;
}
