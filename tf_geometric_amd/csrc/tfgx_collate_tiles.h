// The per-element bodies of minibatch assembly, shared by tfgx_collate.hip (sizes the host knows) and tfgx_collate_static.hip
// (capacities the host knows, live totals read from the table on the device): every live element of either kernel is produced
// by the code below, so the live part of a fixed-shape batch is bit for bit what tfgx_collate writes.
//
// Reference: tf_geometric/data/graph.py:463-560 (BatchGraph.from_graphs).  A launch is cut into SECTIONS of tiles of kTile
// output elements, told apart by the workgroup index alone (wave-uniform, no divergence):
//   feature section : the rows * F floats of out_x                                    (the only wide traffic)
//   node section    : out_node_graph_index[r] and the plans' out_row_ptr[r], r in [0, rows]   (row `rows` only with a plan)
//   edge section    : out_row / out_col / out_edge_graph_index / out_w and the plans' (out_col, out_perm), q in [0, edges)
// The graphs are tiny (tens of nodes) and the batch is ragged, so nothing is indexed by graph: every element finds its slot
// with upper_bound over the B + 1 output offsets — staged in LDS when they fit (kLdsOffsets), read from global memory
// otherwise.  Equal consecutive offsets (empty slots) are skipped by the upper bound.  Offsets into x are 64-bit, the rest is
// int32.  Plain stores only: the output is a pure function of the inputs.
//
// STATIC = false: rows = n_out and edges = e_out, every element is live.
// STATIC = true : rows = n_cap and edges = e_cap; n_live = out_node_ptr[B] and e_live = out_edge_ptr[B] are read on the device.
//   Rows past n_live are dead (x = 0, graph index B, no edges of their own) and the last `sinks` of them are the sinks; edge
//   q >= e_live is a unit self-loop on sink (q - e_live) / sink_degree, and is its own CSR position in both plans: the sinks
//   follow every live row and do not decrease with q, so a stable sort leaves the tail where it is.
#pragma once
#include "tfgx_common.h"
#include "tfgx_host.h"
#include "../../include/tfgx_collate.h"

namespace tfgx {
namespace collate {

constexpr int kTile = TFGX_COLLATE_TILE;               // output elements per workgroup
constexpr int kItems = kTile / kBlock;                 // 4 per thread: one float4 on the vector path
constexpr int kLdsOffsets = 1024;                      // B + 1 <= this: the offsets are searched in LDS (4 KiB)
static_assert(kTile == kBlock * 4, "the vector path moves one float4 per thread and tile");

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
    int32_t B, n_out, e_out;           // STATIC: n_out = n_cap, e_out = e_cap
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
    // STATIC only
    int32_t sinks, sink_degree;        // the last `sinks` rows; at most sink_degree padded edges on each
    int32_t* graph_row_ptr;            // [B + 2]: out_node_ptr[0 .. B], then n_cap
    int32_t edge_tiles;                // the graph section follows the edge section
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

// STATIC: the live totals, held to the capacities whatever the table says (no store leaves the outputs)
__device__ __forceinline__ int32_t live_nodes(const Params& p) { return max(min(p.out_node_ptr[p.B], p.n_out - p.sinks), 0); }
__device__ __forceinline__ int32_t live_edges(const Params& p) { return max(min(p.out_edge_ptr[p.B], p.e_out), 0); }

template <bool VEC4, bool STATIC>
__device__ __forceinline__ void feature_tile(const Params& p, int64_t tile, int32_t* lds)
{
    const int32_t* ptr = stage_offsets(p.out_node_ptr, p.B, lds);
    const int32_t n_live = STATIC ? live_nodes(p) : p.n_out;
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
        if (STATIC && r >= n_live) {                               // a dead row
            if constexpr (VEC4) *reinterpret_cast<float4*>(p.out_x + int64_t(r) * p.out_ldx + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
            else p.out_x[int64_t(r) * p.out_ldx + c] = 0.0f;
            continue;
        }
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

template <bool STATIC>
__device__ __forceinline__ void node_tile(const Params& p, int32_t tile, int32_t* lds)
{
    const int32_t* ptr = (STATIC || p.n_out > 0) ? stage_offsets(p.out_node_ptr, p.B, lds) : nullptr;
    const int32_t n_live = STATIC ? live_nodes(p) : p.n_out;
    const int32_t e_live = STATIC ? live_edges(p) : p.e_out;
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
        if (STATIC && r >= n_live) {
            // a dead row: empty unless it is a sink; sink t holds the padded edges [t, t + 1) * sink_degree of the tail
            p.out_ngi[r] = p.B;
            const int32_t t = max(r - (p.n_out - p.sinks), 0);
            const int64_t before = min(int64_t(p.e_out - e_live), int64_t(t) * p.sink_degree);
            for (int k = 0; k < 2; ++k)
                if (p.plan[k].ds_row_ptr != nullptr) p.plan[k].out_row_ptr[r] = e_live + int32_t(before);
            continue;
        }
        const int32_t j = slot_of(ptr, p.B, r);
        p.out_ngi[r] = j;
        const int32_t src_row = p.src_node_begin[j] + (r - ptr[j]);
        const int32_t shift = p.out_edge_ptr[j] - p.src_edge_begin[j];
        for (int k = 0; k < 2; ++k)
            if (p.plan[k].ds_row_ptr != nullptr) p.plan[k].out_row_ptr[r] = p.plan[k].ds_row_ptr[src_row] + shift;
    }
}

template <bool STATIC>
__device__ __forceinline__ void edge_tile(const Params& p, int32_t tile, int32_t* lds)
{
    const int32_t* ptr = stage_offsets(p.out_edge_ptr, p.B, lds);
    const int32_t e_live = STATIC ? live_edges(p) : p.e_out;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int64_t q64 = int64_t(tile) * kTile + it * kBlock + threadIdx.x;
        if (q64 >= p.e_out) break;
        const int32_t q = int32_t(q64);
        if (STATIC && q >= e_live) {                               // the padded tail: a unit self-loop on its sink
            const int32_t v = p.n_out - p.sinks + (q - e_live) / p.sink_degree;
            p.out_row[q] = v;
            p.out_col[q] = v;
            p.out_egi[q] = p.B;
            if (p.out_w != nullptr) p.out_w[q] = 1.0f;
            for (int k = 0; k < 2; ++k)
                if (p.plan[k].ds_row_ptr != nullptr) {
                    p.plan[k].out_col[q] = v;
                    p.plan[k].out_perm[q] = q;
                }
            continue;
        }
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

inline PlanDev plan_dev(const tfgx_collate_plan* pl)
{
    if (pl == nullptr) return PlanDev{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return PlanDev{pl->ds_row_ptr, pl->ds_col, pl->ds_perm, pl->out_row_ptr, pl->out_col, pl->out_perm};
}

// the null checks of one plan, with the entry point and the member named
inline int check_plan(const char* entry, const char* which, const tfgx_collate_plan* pl, int64_t ds_e, int64_t e_out)
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
        set_error("%s: %s->%s is null", entry, which, bad);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

}  // namespace collate
}  // namespace tfgx
