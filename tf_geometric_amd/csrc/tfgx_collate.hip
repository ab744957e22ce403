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
#include "../../include/tfgx_collate.h"

namespace tfgx {
namespace {

constexpr int kTile = TFGX_COLLATE_TILE;               // output elements per workgroup
constexpr int kItems = kTile / kBlock;                 // 4 per thread: one float4 on the vector path
constexpr int kLdsOffsets = 1024;                      // B + 1 <= this: the offsets are searched in LDS (4 KiB)
static_assert(kTile == kBlock * 4, "the vector path moves one float4 per thread and tile");

constexpr int64_t kMaxSize = (int64_t(1) << 31) - 1;

struct PlanDev {
    const int32_t* ds_row_ptr;
    const int32_t* ds_col;
    const int32_t* ds_perm;
    int32_t* out_row_ptr;
    int32_t* out_col;
    int32_t* out_perm;
};

struct Params {
    const float* ds_x;
    int64_t ds_ldx;
    int32_t F;
    const int32_t* ds_row;
    const int32_t* ds_col;
    const float* ds_w;
    const int32_t* src_node_begin;     // the four table columns
    const int32_t* out_node_ptr;
    const int32_t* src_edge_begin;
    const int32_t* out_edge_ptr;
    int32_t B, n_out, e_out;
    float* out_x;
    int64_t out_ldx;
    int32_t* out_ngi;
    int32_t* out_row;
    int32_t* out_col;
    int32_t* out_egi;
    float* out_w;
    PlanDev plan[2];                   // by destination, by source; ds_row_ptr == nullptr: absent
    int32_t node_items;                // n_out, or n_out + 1 when a plan wants out_row_ptr[n_out]
    int64_t x_tiles;                   // tiles of the feature section
    int32_t node_tiles;
};

// slot of element i: the last j with ptr[j] <= i, ptr[0] = 0 <= i < ptr[B]; never an empty slot
__device__ __forceinline__ int32_t slot_of(const int32_t* ptr, int32_t B, int32_t i)
{
    int32_t lo = 0, hi = B;            // invariant: ptr[lo] <= i < ptr[hi]
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the B + 1 offsets the section searches: LDS copy when it fits, the global column otherwise
__device__ __forceinline__ const int32_t* stage_offsets(const int32_t* __restrict__ g, int32_t B, int32_t* lds)
{
    if (B + 1 > kLdsOffsets) return g;
    for (int32_t j = threadIdx.x; j <= B; j += kBlock) lds[j] = g[j];
    __syncthreads();
    return lds;
}

template <bool VEC4>
__device__ __forceinline__ void feature_tile(const Params& p, int64_t tile, int32_t* lds)
{
    const int32_t* ptr = stage_offsets(p.out_node_ptr, p.B, lds);
    // row width in items: floats, or float4s on the vector path (F, both leading dimensions and both bases allow it)
    const int32_t width = VEC4 ? p.F / 4 : p.F;
    const int64_t total = int64_t(p.n_out) * width;
    const int64_t first = tile * (VEC4 ? kBlock : kTile);          // the tile's first item
    const int64_t row0 = first / width;                            // wave-uniform: one 64-bit division per workgroup
    const int32_t rem0 = int32_t(first - row0 * width);
#pragma unroll
    for (int it = 0; it < (VEC4 ? 1 : kItems); ++it) {
        const int32_t local = it * kBlock + int32_t(threadIdx.x);
        if (first + local >= total) break;
        const int32_t in_row = rem0 + local;                       // < width + kTile: int32
        const int32_t r = int32_t(row0) + in_row / width;
        const int32_t c = in_row % width;
        const int32_t j = slot_of(ptr, p.B, r);
        const int64_t src_row = int64_t(p.src_node_begin[j]) + (r - ptr[j]);
        if constexpr (VEC4) {
            const float4 v = *reinterpret_cast<const float4*>(p.ds_x + src_row * p.ds_ldx + 4 * c);
            *reinterpret_cast<float4*>(p.out_x + int64_t(r) * p.out_ldx + 4 * c) = v;
        } else {
            p.out_x[int64_t(r) * p.out_ldx + c] = p.ds_x[src_row * p.ds_ldx + c];
        }
    }
}

__device__ __forceinline__ void node_tile(const Params& p, int32_t tile, int32_t* lds)
{
    const int32_t* ptr = p.n_out > 0 ? stage_offsets(p.out_node_ptr, p.B, lds) : nullptr;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int64_t r64 = int64_t(tile) * kTile + it * kBlock + threadIdx.x;
        if (r64 >= p.node_items) break;
        const int32_t r = int32_t(r64);
        if (r == p.n_out) {                                        // only reached with a plan: node_items = n_out + 1
            for (int k = 0; k < 2; ++k)
                if (p.plan[k].ds_row_ptr != nullptr) p.plan[k].out_row_ptr[r] = p.e_out;
            break;
        }
        const int32_t j = slot_of(ptr, p.B, r);
        p.out_ngi[r] = j;
        const int32_t src_row = p.src_node_begin[j] + (r - ptr[j]);
        const int32_t shift = p.out_edge_ptr[j] - p.src_edge_begin[j];
        for (int k = 0; k < 2; ++k)
            if (p.plan[k].ds_row_ptr != nullptr) p.plan[k].out_row_ptr[r] = p.plan[k].ds_row_ptr[src_row] + shift;
    }
}

__device__ __forceinline__ void edge_tile(const Params& p, int32_t tile, int32_t* lds)
{
    const int32_t* ptr = stage_offsets(p.out_edge_ptr, p.B, lds);
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int64_t q64 = int64_t(tile) * kTile + it * kBlock + threadIdx.x;
        if (q64 >= p.e_out) break;
        const int32_t q = int32_t(q64);
        const int32_t j = slot_of(ptr, p.B, q);
        const int32_t s = p.src_edge_begin[j] + (q - ptr[j]);
        const int32_t node_shift = p.out_node_ptr[j] - p.src_node_begin[j];
        const int32_t edge_shift = ptr[j] - p.src_edge_begin[j];
        p.out_row[q] = p.ds_row[s] + node_shift;
        p.out_col[q] = p.ds_col[s] + node_shift;
        p.out_egi[q] = j;
        if (p.out_w != nullptr) p.out_w[q] = p.ds_w != nullptr ? p.ds_w[s] : 1.0f;
        for (int k = 0; k < 2; ++k)
            if (p.plan[k].ds_row_ptr != nullptr) {
                p.plan[k].out_col[q] = p.plan[k].ds_col[s] + node_shift;
                p.plan[k].out_perm[q] = p.plan[k].ds_perm[s] + edge_shift;
            }
    }
}

template <bool VEC4>
__global__ void __launch_bounds__(kBlock) collate_kernel(const Params p)
{
    __shared__ int32_t lds[kLdsOffsets];
    const int64_t b = blockIdx.x;
    if (b < p.x_tiles) feature_tile<VEC4>(p, b, lds);
    else if (b < p.x_tiles + p.node_tiles) node_tile(p, int32_t(b - p.x_tiles), lds);
    else edge_tile(p, int32_t(b - p.x_tiles - p.node_tiles), lds);
}

int check_plan(const char* which, const tfgx_collate_plan* pl, int64_t ds_e, int64_t e_out)
{
    if (pl == nullptr) return TFGX_OK;
    const char* bad = nullptr;
    if (pl->ds_row_ptr == nullptr) bad = "ds_row_ptr";
    else if (pl->out_row_ptr == nullptr) bad = "out_row_ptr";
    else if (ds_e > 0 && pl->ds_col == nullptr) bad = "ds_col";
    else if (ds_e > 0 && pl->ds_perm == nullptr) bad = "ds_perm";
    else if (e_out > 0 && pl->out_col == nullptr) bad = "out_col";
    else if (e_out > 0 && pl->out_perm == nullptr) bad = "out_perm";
    if (bad != nullptr) {
        set_error("tfgx_collate: %s->%s is null", which, bad);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

PlanDev plan_dev(const tfgx_collate_plan* pl)
{
    if (pl == nullptr) return PlanDev{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return PlanDev{pl->ds_row_ptr, pl->ds_col, pl->ds_perm, pl->out_row_ptr, pl->out_col, pl->out_perm};
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
    const struct { const char* name; int64_t v; } sizes[] = {{"ds_ldx", a->ds_ldx}, {"F", a->F}, {"ds_n", a->ds_n}, {"ds_e", a->ds_e},
                                                             {"B", a->B}, {"n_out", a->n_out}, {"e_out", a->e_out},
                                                             {"out_ldx", a->out_ldx}};
    for (const auto& s : sizes) {
        if (s.v < 0) {
            set_error("tfgx_collate: negative size (%s = %lld)", s.name, (long long)s.v);
            return TFGX_ERR_INVALID_ARG;
        }
        if (s.v >= kMaxSize) {
            set_error("tfgx_collate: %s = %lld does not fit int32", s.name, (long long)s.v);
            return TFGX_ERR_INVALID_ARG;
        }
    }
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
    if (int rc = check_plan("plan", a->plan, a->ds_e, a->e_out)) return rc;
    if (int rc = check_plan("plan_t", a->plan_t, a->ds_e, a->e_out)) return rc;

    Params p;
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
