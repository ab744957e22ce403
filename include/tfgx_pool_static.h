/*
 * tfgx_static_pool — one fixed-shape SAGPool level: a static batch (include/tfgx_collate_static.h) in, a static batch out, at
 * sizes the host knows.  Nothing is read back and nothing is sorted by destination, so a hierarchical graph classifier over
 * fixed-shape batches is a fixed launch sequence that a hipGraph can replay.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/nn/pool/topk_pool.py:6-87 (the selection), tf_geometric/nn/pool/sag_pool.py:7-45 (the level) and
 * tf_geometric/data/graph.py:276-359 (BatchGraph.sample_new_graph_by_node_index: the induced subgraph).
 *
 * The parent batch has B slots, n_cap rows (the last `sinks` = P of them the sinks), e_cap edges, graph_row_ptr [B + 2] (the
 * slots' row offsets, then n_live, closed with n_cap) and counts [4].  The pooled batch has the same B, e_cap, P and sink degree
 * d, and n_cap' = m_max + P rows, where m_max bounds the kept nodes of any batch (host arithmetic: DESIGN.md 2.27).
 *
 * Graph g of n_g = graph_row_ptr[g + 1] - graph_row_ptr[g] nodes keeps k_g = min(k, n_g), or
 * min(n_g, (int)ceilf((float)n_g * ratio)) — the rule of tfgx_segment_topk.  Its nodes are ranked by score descending, equal
 * scores in row order, -0.0 equal to +0.0, NaNs where tfgx_segment_topk puts them (the same 32-bit key).  With m_live the sum of
 * k_g and e_kept the number of parent edges whose two endpoints are kept, the layout is
 *   pooled_row_ptr [B + 2] : the exclusive sums of k_g over the slots, then m_live, closed with n_cap';
 *   node_index [n_cap']    : pooled row -> parent row; rows [pooled_row_ptr[g], pooled_row_ptr[g + 1]) are slot g's kept nodes in
 *                            rank order; rows [m_live, n_cap') hold -1;
 *   node_map [n_cap]       : parent row -> pooled row, -1 for a row that is not kept (every dead parent row);
 *   node_graph_index [n_cap'] : the slot of a live pooled row, B for a dead one;
 *   edges [0, e_kept)      : the kept edges in parent order, relabelled through node_map, with edge_id = the parent position,
 *                            the parent's edge_graph_index and weight (1.0f without parent weights);
 *   edges [e_kept, e_cap)  : edge q is a unit self-loop on sink t = (q - e_kept) / d: row = col = n_cap' - P + t, weight 1.0f,
 *                            edge_id = -1, edge_graph_index = B.  The parent's own padded self-loops sit on dead rows and drop
 *                            out by themselves;
 *   the two plans          : what tfgx_build_csr_by_dst gives for the emitted [2, e_cap] list and for its flip.  Pooled row
 *                            j < m_live is parent row node_index[j] walked in CSR order (a stable sort keeps the parent order
 *                            within a row), dead non-sink rows are empty, sink rows have a closed form, the padded tail is the
 *                            identity — no sort;
 *   counts [4]             : live graphs (copied), m_live, e_kept, flags: the parent's flags carried on, and the two bits below.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code with
 * text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.  Zero-size
 * calls succeed.  No float atomics and no global atomics: every output is a pure function of the inputs.  Every index read
 * from device memory is held to its array's bounds before it is used as an address, and every store to the capacities.
 */
#ifndef TFGX_POOL_STATIC_H
#define TFGX_POOL_STATIC_H

#include "tfgx_collate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_STATIC_POOL_ABI_VERSION 1
int tfgx_static_pool_version(void);   /* the TFGX_STATIC_POOL_ABI_VERSION the library was built with */

/* The longest graph tfgx_static_pool_select ranks: its 8-byte keys live in LDS (32 KiB). */
#define TFGX_STATIC_POOL_MAX_GRAPH_NODES 4096

/* Bits of counts[3], beside TFGX_STATIC_BATCH_BAD_ID (1) and TFGX_STATIC_BATCH_OVERFLOW (2) of the parent. */
#define TFGX_STATIC_POOL_CLAMPED 4       /* the kept nodes exceeded m_max and were cut off: the capacities are not this batch's */
#define TFGX_STATIC_POOL_TOO_LONG 8      /* a graph of more than TFGX_STATIC_POOL_MAX_GRAPH_NODES nodes: it keeps no node */

/* The most slots the one-workgroup scan of tfgx_static_pool_table covers. */
#define TFGX_STATIC_POOL_MAX_SLOTS 1048576

/* (a) The pooled table, ONE launch (one workgroup scans the B slots).
 *   graph_row_ptr [B + 2], parent_counts [4] : the parent's
 *   k >= 0: keep min(k, n_g); k < 0: keep by `ratio` (>= 0)
 *   m_max, n_cap_out : the pooled capacities (n_cap_out >= m_max)
 *   pooled_row_ptr [B + 2], counts [4] : written (counts[2] = 0 until tfgx_static_pool_edges fills it)
 * Refused: a null pointer, B < 0 or B > TFGX_STATIC_POOL_MAX_SLOTS, m_max or n_cap_out negative or not fitting int32,
 * n_cap_out < m_max, k < 0 with a ratio that is negative or NaN. */
int tfgx_static_pool_table(const int32_t* graph_row_ptr, const int32_t* parent_counts, int64_t B, int32_t k, float ratio,
                           int64_t m_max, int64_t n_cap_out, int32_t* pooled_row_ptr, int32_t* counts, tfgx_stream_t stream);

/* (b) The selection, ONE launch: one workgroup per slot ranks the slot's nodes in LDS; further workgroups fill
 * node_index / node_graph_index of the dead pooled rows and node_map of the dead parent rows.
 *   score [n_cap] float32, graph_row_ptr [B + 2], pooled_row_ptr [B + 2] (from tfgx_static_pool_table)
 *   n_cap, sinks : the parent's rows and sinks;  n_cap_out : the pooled rows
 *   node_index [n_cap_out], node_graph_index [n_cap_out], node_map [n_cap] : written, every entry
 * Refused: a null pointer that the sizes need, a negative size or one not fitting int32, B > TFGX_STATIC_POOL_MAX_SLOTS,
 * sinks > n_cap. */
int tfgx_static_pool_select(const float* score, const int32_t* graph_row_ptr, const int32_t* pooled_row_ptr, int64_t B,
                            int64_t n_cap, int64_t sinks, int64_t n_cap_out, int32_t* node_index, int32_t* node_graph_index,
                            int32_t* node_map, tfgx_stream_t stream);

typedef struct tfgx_static_pool_args {
    /* the parent batch */
    const int32_t* row;              /* [e_cap] edge_index[0] */
    const int32_t* col;              /* [e_cap] edge_index[1] */
    const float* w;                  /* [e_cap] or NULL (all ones) */
    const int32_t* edge_graph_index; /* [e_cap] */
    int64_t n_cap;                   /* parent rows */
    int64_t e_cap;                   /* edges, of the parent and of the pooled batch */
    int64_t B;
    int64_t sinks;                   /* P */
    int64_t sink_degree;             /* d */
    /* the selection (tfgx_static_pool_table, tfgx_static_pool_select) */
    const int32_t* node_map;         /* [n_cap] */
    const int32_t* node_index;       /* [n_cap_out] */
    const int32_t* pooled_row_ptr;   /* [B + 2] */
    int64_t n_cap_out;               /* pooled rows, the P sinks included */
    /* the outputs */
    int32_t* out_row;                /* [e_cap] */
    int32_t* out_col;                /* [e_cap] */
    int32_t* out_edge_id;            /* [e_cap] */
    int32_t* out_edge_graph_index;   /* [e_cap] */
    float* out_w;                    /* [e_cap] or NULL (not written) */
    const tfgx_collate_plan* plan;   /* by destination: ds_* the parent's [n_cap + 1] / [e_cap], out_* [n_cap_out + 1] / [e_cap] */
    const tfgx_collate_plan* plan_t; /* by source */
    int32_t* counts;                 /* [4]: counts[2] = e_kept is written */
    void* workspace;
    size_t workspace_bytes;          /* at least tfgx_static_pool_edges_workspace_bytes(n_cap_out, e_cap) */
} tfgx_static_pool_args;

size_t tfgx_static_pool_edges_workspace_bytes(int64_t n_cap_out, int64_t e_cap);

/* (c) Pooled edges and both plans: a FIXED sequence of four launches (count, scan, emit edges, emit plans) with no host read
 * between them; the kept total stays on the device.  Refused on the host, with the member named: a null member that the sizes
 * need (both plans, counts, the selection and the workspace always), a negative size, a size not fitting int32,
 * sink_degree < 1, sinks > n_cap_out, sinks > n_cap, sinks * sink_degree < e_cap, a workspace that is too small. */
int tfgx_static_pool_edges(const tfgx_static_pool_args* args, tfgx_stream_t stream);

/* (d) Pooled features: out[i, :] = idx[i] >= 0 ? x[idx[i], :] * s[idx[i]] : 0 for i in [0, M) (s == NULL: no scaling).  The row
 * max(idx[i], 0) is loaded whatever idx[i] is (a clamped load, not a predicated one) and replaced by zeros afterwards: -1 is
 * never an address.  idx[i] is held below n as well.  The backward is tfgx_gather_scale_rows_backward_f32 (tfgx.h) through
 * node_map.  Refused: negative sizes, ldx < F or ldo < F, a null pointer with M, F > 0, n == 0 with M, F > 0. */
int tfgx_static_pool_gather_scale_rows_f32(const float* x, int64_t ldx, int64_t n, const int32_t* idx, const float* s, int64_t M,
                                           int64_t F, float* out, int64_t ldo, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_POOL_STATIC_H */
