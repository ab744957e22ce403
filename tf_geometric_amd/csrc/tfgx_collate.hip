// Minibatch assembly out of a packed, device-resident dataset (include/tfgx_collate.h): one launch, no sort.
//
// Reference: tf_geometric/data/graph.py:463-560 (BatchGraph.from_graphs).  The launch is cut into three SECTIONS of tiles of
// kTile output elements, told apart by the workgroup index alone (wave-uniform, no divergence):
//   feature section : the n_out * F floats of out_x                                   (the only wide traffic)
//   node section    : out_node_graph_index[r] and the plans' out_row_ptr[r], r in [0, n_out]   (row n_out only with a plan)
//   edge section    : out_row / out_col / out_edge_graph_index / out_w and the plans' (out_col, out_perm), q in [0, e_out)
// The graphs are tiny (tens of nodes) and the batch is ragged, so nothing is indexed by graph: every element finds its slot
// with upper_bound over the B + 1 output offsets — staged in LDS when they fit (kLdsOffsets), read from global memory
// otherwise.  Equal consecutive offsets (empty slots) are skipped by the upper bound.  Offsets into x are 64-bit, the rest is
// int32.  Plain stores only: the output is a pure function of the inputs.
#include "tfgx_common.h"
#include "tfgx_collate_tiles.h"
#include "../../include/tfgx_collate.h"

namespace tfgx {
namespace {

using namespace collate;      // the sections' per-element bodies (shared with tfgx_collate_static.hip), all elements live

template <bool VEC4>
__global__ void __launch_bounds__(kBlock) collate_kernel(const Params p)
{
    __shared__ int32_t lds[kLdsOffsets];
    const int64_t b = blockIdx.x;
    if (b < p.x_tiles) feature_tile<VEC4, false>(p, b, lds);
    else if (b < p.x_tiles + p.node_tiles) node_tile<false>(p, int32_t(b - p.x_tiles), lds);
    else edge_tile<false>(p, int32_t(b - p.x_tiles - p.node_tiles), lds);
}

}  // namespace
}  // namespace tfgx

using namespace tfgx;

extern "C" int tfgx_collate_version(void) { return TFGX_COLLATE_ABI_VERSION; }
extern "C" int tfgx_collate_tile(void) { return TFGX_COLLATE_TILE; }

extern "C" int tfgx_collate(const tfgx_collate_args* a, tfgx_stream_t stream_)
{
    TFGX_RANGE();
    hipStream_t stream = as_stream(stream_);
    TFGX_REQUIRE(a != nullptr, "args is null");
    const NamedSize sizes[] = {{"ds_ldx", a->ds_ldx}, {"F", a->F}, {"ds_n", a->ds_n}, {"ds_e", a->ds_e}, {"B", a->B},
                               {"n_out", a->n_out}, {"e_out", a->e_out}, {"out_ldx", a->out_ldx}};
    if (int rc = check_sizes("tfgx_collate", sizes)) return rc;
    if (a->n_out > a->ds_n * a->B) {       // both factors are below 2^31: no overflow
        set_error("tfgx_collate: n_out = %lld is more than B = %lld graphs of a dataset of ds_n = %lld nodes can hold",
                  (long long)a->n_out, (long long)a->B, (long long)a->ds_n);
        return TFGX_ERR_INVALID_ARG;
    }
    if (a->e_out > a->ds_e * a->B) {
        set_error("tfgx_collate: e_out = %lld is more than B = %lld graphs of a dataset of ds_e = %lld edges can hold",
                  (long long)a->e_out, (long long)a->B, (long long)a->ds_e);
        return TFGX_ERR_INVALID_ARG;
    }
    const bool has_x = a->n_out > 0 && a->F > 0;
    if (has_x && a->ds_ldx < a->F) {
        set_error("tfgx_collate: ds_ldx = %lld is smaller than F = %lld", (long long)a->ds_ldx, (long long)a->F);
        return TFGX_ERR_INVALID_ARG;
    }
    if (has_x && a->out_ldx < a->F) {
        set_error("tfgx_collate: out_ldx = %lld is smaller than F = %lld", (long long)a->out_ldx, (long long)a->F);
        return TFGX_ERR_INVALID_ARG;
    }
    const char* bad = nullptr;
    if ((a->n_out > 0 || a->e_out > 0) && a->table == nullptr) bad = "table";
    else if (has_x && a->ds_x == nullptr) bad = "ds_x";
    else if (has_x && a->out_x == nullptr) bad = "out_x";
    else if (a->n_out > 0 && a->out_node_graph_index == nullptr) bad = "out_node_graph_index";
    else if (a->e_out > 0 && a->ds_row == nullptr) bad = "ds_row";
    else if (a->e_out > 0 && a->ds_col == nullptr) bad = "ds_col";
    else if (a->e_out > 0 && a->out_row == nullptr) bad = "out_row";
    else if (a->e_out > 0 && a->out_col == nullptr) bad = "out_col";
    else if (a->e_out > 0 && a->out_edge_graph_index == nullptr) bad = "out_edge_graph_index";
    if (bad != nullptr) {
        set_error("tfgx_collate: %s is null", bad);
        return TFGX_ERR_INVALID_ARG;
    }
    if (int rc = check_plan("tfgx_collate", "plan", a->plan, a->ds_e, a->e_out)) return rc;
    if (int rc = check_plan("tfgx_collate", "plan_t", a->plan_t, a->ds_e, a->e_out)) return rc;

    Params p = {};
    p.ds_x = a->ds_x;
    p.ds_ldx = a->ds_ldx;
    p.F = int32_t(a->F);
    p.ds_row = a->ds_row;
    p.ds_col = a->ds_col;
    p.ds_w = a->ds_w;
    const int64_t stride = a->B + 1;
    p.src_node_begin = a->table;
    p.out_node_ptr = a->table == nullptr ? nullptr : a->table + stride;
    p.src_edge_begin = a->table == nullptr ? nullptr : a->table + 2 * stride;
    p.out_edge_ptr = a->table == nullptr ? nullptr : a->table + 3 * stride;
    p.B = int32_t(a->B);
    p.n_out = int32_t(a->n_out);
    p.e_out = int32_t(a->e_out);
    p.out_x = a->out_x;
    p.out_ldx = a->out_ldx;
    p.out_ngi = a->out_node_graph_index;
    p.out_row = a->out_row;
    p.out_col = a->out_col;
    p.out_egi = a->out_edge_graph_index;
    p.out_w = a->out_w;
    p.plan[0] = plan_dev(a->plan);
    p.plan[1] = plan_dev(a->plan_t);
    const bool with_plan = a->plan != nullptr || a->plan_t != nullptr;
    p.node_items = int32_t(a->n_out + (with_plan ? 1 : 0));

    const bool vec4 = has_x && a->F % 4 == 0 && a->ds_ldx % 4 == 0 && a->out_ldx % 4 == 0 && aligned_to(a->ds_x, 16) &&
                      aligned_to(a->out_x, 16);
    const int64_t x_items = has_x ? a->n_out * (vec4 ? a->F / 4 : a->F) : 0;
    const int64_t x_per_tile = vec4 ? kBlock : kTile;              // a tile is kTile floats either way
    p.x_tiles = (x_items + x_per_tile - 1) / x_per_tile;
    p.node_tiles = int32_t((int64_t(p.node_items) + kTile - 1) / kTile);
    const int64_t edge_tiles = (a->e_out + kTile - 1) / kTile;
    const int64_t grid = p.x_tiles + p.node_tiles + edge_tiles;
    if (grid == 0) return TFGX_OK;
    if (grid >= kMaxSize) {
        set_error("tfgx_collate: n_out * F = %lld elements need more workgroups than one launch has", (long long)(a->n_out * a->F));
        return TFGX_ERR_INVALID_ARG;
    }
    if (vec4) collate_kernel<true><<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(p);
    else collate_kernel<false><<<static_cast<unsigned>(grid), kBlock, 0, stream>>>(p);
    TFGX_LAUNCH_CHECK("collate_kernel");
    return TFGX_OK;
}
