/*
 * tfgx_collate — assemble a minibatch of whole graphs out of a device-resident dataset, with its CSR plans, without a sort.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/data/graph.py:463-560 (BatchGraph.from_graphs: concatenate x, edge_index + node offset, edge_weight,
 * and fill node_graph_index / edge_graph_index with the position of each graph in the batch).
 *
 * The dataset is PACKED: the nodes of graph g are rows [node_ptr[g], node_ptr[g+1]) of ds_x, its edges are entries
 * [edge_ptr[g], edge_ptr[g+1]) of (ds_row, ds_col), and the endpoints are dataset-global node ids, so every edge of a graph
 * stays inside that graph's node range.  A batch of whole graphs is block-diagonal, and tfgx_build_csr_by_dst is a stable sort
 * by (row, edge id); so the CSR plan of a batch IS the concatenation of its graphs' pieces of the DATASET's plan with the node
 * and edge offsets exchanged — bit for bit what a rebuild of the emitted list gives (the argument of tfgx_dropedge.h).  The
 * CSR positions of graph g in the dataset's plan are [edge_ptr[g], edge_ptr[g+1]) as well, by destination and by source.
 *
 * The caller describes the batch with a table of four int32 columns of B + 1 entries each, on the device
 * (table[c * (B + 1) + j], slot j = position of the graph in the batch):
 *   column 0  src_node_begin[j] : node_ptr[graph of slot j]                (entry B unused)
 *   column 1  out_node_ptr[j]   : first output row of slot j;  [B] = n_out
 *   column 2  src_edge_begin[j] : edge_ptr[graph of slot j]                (entry B unused)
 *   column 3  out_edge_ptr[j]   : first output edge of slot j; [B] = e_out
 * out_node_ptr / out_edge_ptr are non-decreasing from 0; a slot may be empty (graphs without nodes or without edges) and a
 * graph may appear in several slots.  The table's consistency with the dataset is the caller's contract: it is not read on
 * the host.  With j = the slot of output row r (of output edge q) and s = src_edge_begin[j] + q - out_edge_ptr[j]:
 *   out_x[r]                = ds_x[src_node_begin[j] + r - out_node_ptr[j]]
 *   out_node_graph_index[r] = j,   out_edge_graph_index[q] = j
 *   out_row / out_col [q]   = ds_row / ds_col [s] - src_node_begin[j] + out_node_ptr[j]
 *   out_w[q]                = ds_w[s]   (1.0f when ds_w is NULL)
 *   plan: out_row_ptr[r]    = ds_row_ptr[src row] - src_edge_begin[j] + out_edge_ptr[j],  out_row_ptr[n_out] = e_out
 *         out_col[q]        = ds_col[s]  - src_node_begin[j] + out_node_ptr[j]
 *         out_perm[q]       = ds_perm[s] - src_edge_begin[j] + out_edge_ptr[j]
 *
 * ONE launch per call whatever B is: work is indexed by flat output element, in tiles of TFGX_COLLATE_TILE elements per
 * workgroup; the slot of an element is upper_bound(out_ptr, i) - 1 (so it never lands on an empty slot), searched in LDS when
 * the B + 1 offsets fit there and in global memory otherwise.  No atomics, nothing allocated here, no synchronisation: the
 * output is a pure function of the inputs.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error()).
 */
#ifndef TFGX_COLLATE_H
#define TFGX_COLLATE_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_COLLATE_ABI_VERSION 1
int tfgx_collate_version(void);   /* the TFGX_COLLATE_ABI_VERSION the library was built with */

/* Output elements per workgroup: feature ELEMENTS (floats), node rows and edges are each cut into tiles of this size. */
#define TFGX_COLLATE_TILE 1024
int tfgx_collate_tile(void);      /* the TFGX_COLLATE_TILE the library was built with */

/* One CSR plan of the PACKED DATASET (tfgx_build_csr_by_dst layout over all its ds_n nodes and ds_e edges) and where the
 * batch's plan goes: by destination = build(ds_row, ds_col), by source = build(ds_col, ds_row).
 * out_row_ptr [n_out + 1], out_col [e_out], out_perm [e_out]. */
typedef struct tfgx_collate_plan {
    const int32_t* ds_row_ptr;   /* [ds_n + 1] */
    const int32_t* ds_col;       /* [ds_e] */
    const int32_t* ds_perm;      /* [ds_e] CSR position -> dataset edge id */
    int32_t* out_row_ptr;
    int32_t* out_col;
    int32_t* out_perm;
} tfgx_collate_plan;

typedef struct tfgx_collate_args {
    /* the packed dataset */
    const float* ds_x;           /* [ds_n, F] rows on leading dimension ds_ldx (floats) */
    int64_t ds_ldx;
    int64_t F;
    const int32_t* ds_row;       /* [ds_e] edge_index[0] in dataset-global node ids */
    const int32_t* ds_col;       /* [ds_e] edge_index[1] */
    const float* ds_w;           /* [ds_e] or NULL (all ones) */
    int64_t ds_n;                /* nodes of the whole dataset */
    int64_t ds_e;                /* edges of the whole dataset */
    /* the batch */
    const int32_t* table;        /* [4, B + 1] on the device, see above */
    int64_t B;
    int64_t n_out;
    int64_t e_out;
    /* the outputs */
    float* out_x;                /* [n_out, F] rows on leading dimension out_ldx */
    int64_t out_ldx;
    int32_t* out_node_graph_index;   /* [n_out] */
    int32_t* out_row;            /* [e_out] */
    int32_t* out_col;            /* [e_out] */
    int32_t* out_edge_graph_index;   /* [e_out] */
    float* out_w;                /* [e_out] or NULL (not written) */
    /* the plans: NULL, or the dataset's plan and the outputs for the batch's */
    const tfgx_collate_plan* plan;     /* by destination */
    const tfgx_collate_plan* plan_t;   /* by source */
} tfgx_collate_args;

/* Asynchronous on `stream`, one kernel launch.  Refused on the host, before any device work, with the member named: a null
 * member that the sizes need, a negative size, a size that does not fit int32, ds_ldx < F or out_ldx < F, n_out > ds_n * B,
 * e_out > ds_e * B.  B == 0, n_out == 0 and e_out == 0 succeed and write only what exists: a plan's out_row_ptr[0 .. n_out]
 * is written whenever the plan is given. */
int tfgx_collate(const tfgx_collate_args* args, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_COLLATE_H */
