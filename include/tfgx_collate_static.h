/*
 * tfgx_static_batch — the fixed-shape form of tfgx_collate.h: a batch of B slots whose graph ids live in device memory,
 * assembled into outputs whose sizes are capacities the host knows, with inert padding and all plans.  Nothing is read back, so
 * ids -> batch -> forward -> backward -> optimizer step is a fixed launch sequence that a hipGraph can replay.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/data/graph.py:463-560 (BatchGraph.from_graphs) and demo/demo_mean_pool.py (a batch per step).
 *
 * Capacities (host arithmetic): max_nodes and max_edges bound the live totals of a batch; with a sink degree d >= 1 there are
 * P = max(1, ceil(max_edges / d)) sink rows, n_cap = max_nodes + P rows and e_cap = max_edges edges.
 *
 * Live slots.  ids int32 [B]; slot j is IN RANGE when 0 <= ids[j] < G.  Node and edge counts are cumulated over the in-range
 * slots in slot order; slot j is LIVE when it is in range and both cumulated totals through j stay within max_nodes and
 * max_edges (the totals only grow, so an overflow drops a suffix of the in-range slots).  Every other slot is an empty graph.
 * An id outside [-1, G) raises TFGX_STATIC_BATCH_BAD_ID (it is compared only, never used as an index); a slot dropped for
 * overflow raises TFGX_STATIC_BATCH_OVERFLOW.
 *
 * The layout, with n_live / e_live the live totals:
 *   rows  [0, n_live), edges [0, e_live) : what tfgx_collate writes for the live ids in slot order, bit for bit (the same
 *       per-element code), with the SLOT number in out_node_graph_index / out_edge_graph_index;
 *   rows  [n_live, n_cap) : out_x = 0, out_node_graph_index = B (slot B is the dead graph: the batch has B + 1 graphs); the
 *       last P rows are the sinks, always dead because n_live <= max_nodes;
 *   edges [e_live, e_cap) : edge q is a unit self-loop on sink t = (q - e_live) / d, row = col = n_cap - P + t, weight 1.0f,
 *       out_edge_graph_index = B; no sink has more than d edges;
 *   the two plans are what tfgx_build_csr_by_dst gives for the emitted [2, e_cap] list and its flip: the live part from the
 *       dataset's plans with the offsets exchanged, dead non-sink rows empty, the padded tail the identity (its rows follow
 *       every live row and do not decrease with q, so a stable sort leaves it in place);
 *   graph_row_ptr [B + 2] = out_node_ptr[0 .. B], n_cap : the row_ptr of the graph plan over B + 1 graphs (identity columns).
 *
 * Names: the functions and macros of this header are tfgx_static_batch* / TFGX_STATIC_BATCH_* although the file is
 * tfgx_collate_static.h: names containing "collate" are kept for the table of tfgx_collate.h (tests/test_collate_abi.py).
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.
 * Zero-size calls succeed.  tfgx_static_batch uses no atomics; tfgx_static_batch_table uses integer LDS atomics (add / or,
 * both commutative) only: every output is a pure function of the inputs.
 */
#ifndef TFGX_COLLATE_STATIC_H
#define TFGX_COLLATE_STATIC_H

#include "tfgx_collate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_STATIC_BATCH_ABI_VERSION 1
int tfgx_static_batch_version(void);   /* the TFGX_STATIC_BATCH_ABI_VERSION the library was built with */

/* A dead slot of `ids`. */
#define TFGX_STATIC_BATCH_DEAD (-1)

/* Bits of counts[3]. */
#define TFGX_STATIC_BATCH_BAD_ID 1       /* an id that is neither TFGX_STATIC_BATCH_DEAD nor in [0, G) */
#define TFGX_STATIC_BATCH_OVERFLOW 2     /* an in-range slot dropped because the batch would exceed max_nodes / max_edges */

/* The most slots the one-workgroup scan of tfgx_static_batch_table covers. */
#define TFGX_STATIC_BATCH_MAX_SLOTS 1048576

/* The table of a batch, ONE launch (one workgroup scans the B slots).
 *   ids [B], node_ptr / edge_ptr [G + 1] (the store's per-graph offsets, non-decreasing from 0, as int32)
 *   table [4, B + 1] : the four columns of tfgx_collate.h (src_node_begin, out_node_ptr, src_edge_begin, out_edge_ptr) with
 *                      every slot that is not live an empty one; out_node_ptr[B] = n_live, out_edge_ptr[B] = e_live
 *   live_mask [B]    : one byte per slot, 1 = live
 *   counts [4]       : live graphs, n_live, e_live, flags (written, not OR-ed: the caller need not zero it)
 * Refused: a null pointer (ids, node_ptr, edge_ptr, table, live_mask, counts), B < 0 or B > TFGX_STATIC_BATCH_MAX_SLOTS,
 * G, max_nodes or max_edges negative or not fitting int32.  B == 0 needs no ids, no offsets and no mask, and writes the
 * one-column table (zeros) and counts (zeros) where both are given; with neither it launches nothing. */
int tfgx_static_batch_table(const int32_t* ids, int64_t B, const int32_t* node_ptr, const int32_t* edge_ptr, int64_t G,
                            int64_t max_nodes, int64_t max_edges, int32_t* table, uint8_t* live_mask, int32_t* counts,
                            tfgx_stream_t stream);

typedef struct tfgx_static_batch_args {
    /* the packed dataset (tfgx_collate_args) */
    const float* ds_x;           /* [ds_n, F] rows on leading dimension ds_ldx (floats) */
    int64_t ds_ldx;
    int64_t F;
    const int32_t* ds_row;       /* [ds_e] edge_index[0] in dataset-global node ids */
    const int32_t* ds_col;       /* [ds_e] edge_index[1] */
    const float* ds_w;           /* [ds_e] or NULL (all ones) */
    int64_t ds_n;
    int64_t ds_e;
    /* the batch: the table tfgx_static_batch_table wrote, on the device */
    const int32_t* table;        /* [4, B + 1] */
    int64_t B;
    /* the capacities */
    int64_t n_cap;               /* rows, the sinks included */
    int64_t e_cap;               /* edges */
    int64_t sinks;               /* P: the last P rows */
    int64_t sink_degree;         /* d: padded edges per sink, at most */
    /* the outputs */
    float* out_x;                /* [n_cap, F] rows on leading dimension out_ldx */
    int64_t out_ldx;
    int32_t* out_node_graph_index;   /* [n_cap] */
    int32_t* out_row;            /* [e_cap] */
    int32_t* out_col;            /* [e_cap] */
    int32_t* out_edge_graph_index;   /* [e_cap] */
    float* out_w;                /* [e_cap] or NULL (not written) */
    const tfgx_collate_plan* plan;     /* by destination: out_row_ptr [n_cap + 1], out_col / out_perm [e_cap] */
    const tfgx_collate_plan* plan_t;   /* by source */
    int32_t* graph_row_ptr;      /* [B + 2] */
} tfgx_static_batch_args;

/* Asynchronous on `stream`, ONE launch whose grid the capacities size; n_live / e_live are read from the table on the device
 * (and held to n_cap - sinks / e_cap there, so no store leaves the outputs whatever the table holds).  Refused on the host,
 * before any device work, with the member named: a null member that the sizes need (table, both plans and graph_row_ptr
 * always), a negative size, a size that does not fit int32, sink_degree < 1, sinks > n_cap, sinks * sink_degree < e_cap,
 * ds_ldx < F or out_ldx < F.  n_cap == 0 with e_cap == 0 succeeds: it writes out_row_ptr[0] and graph_row_ptr only, and
 * with neither plan nor graph_row_ptr given it launches nothing. */
int tfgx_static_batch(const tfgx_static_batch_args* args, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_COLLATE_STATIC_H */
