/*
 * tfgx_rows3d — node rows to the dense [G, k, F] tensor of a batch of graphs in ONE launch: utils.convert_x_to_3d (the plain
 * mode) and the SortPool readout nn.sort_pool_3d (the sort mode), also on fixed-shape batches.  G * k output rows whatever the
 * data is: nothing is read back, so both modes can be captured in a hipGraph.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/utils/graph_utils.py:215-249 (convert_x_to_3d), tf_geometric/nn/pool/sort_pool.py:7-35 and
 * tf_geometric/nn/pool/topk_pool.py:6-87 (the selection).
 *
 * Graph g owns the positions [seg_ptr[g], seg_ptr[g + 1]) of the graph plan — the CSR over graphs the readouts use (row_ptr
 * and col of the plan over node_graph_index), or graph_row_ptr with identity nodes on a static batch.  The node at position p
 * is seg_node[p], or p itself when seg_node is NULL.  With n_g the positions of graph g:
 *   plain mode (key == NULL): slot j of graph g is the node at position seg_ptr[g] + j;
 *   sort mode  (key != NULL): the nodes of graph g are ranked by descending_bits(key[node * ldkey]) << 32 | position within the
 *                             graph — the 64-bit key of tfgx_segment_topk and tfgx_static_pool_select: key descending, equal
 *                             keys in plan order, -0.0 equal to +0.0, NaNs where tfgx_segment_topk puts them.  Slot j is the
 *                             node of rank j.
 *   out[g * k + j, :]    = x[node, :] for j < min(n_g, k), exact zeros otherwise: every row of out is written;
 *   slot_node[g * k + j] = that node, or -1;
 *   node_slot[n]         = the slot g * k + j of node n, or -1 (cut off by k, or listed by no graph): every entry of [0, n_rows)
 *                          is written.  node_slot exists for the backward, which needs no kernel of its own:
 *                          dx = tfgx_static_pool_gather_scale_rows_f32(dOut, idx = node_slot, s = NULL) writes every row of dx
 *                          exactly once, as a copy or as zeros — no atomics, the same bits on every run.
 *
 * The sort mode ranks a graph in LDS and so takes graphs of at most TFGX_STATIC_POOL_MAX_GRAPH_NODES (4096) nodes.  A longer
 * one is an ordinary input: its k rows are zero, its slots and its nodes hold -1, and *flags says so.  The plain mode has no
 * cap.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code with
 * text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.  Zero-size
 * calls succeed.  No atomics: every output is a pure function of the inputs.  Every index read from device memory is held to
 * its array's bounds before it is used as an address; loads are clamped and then selected, never predicated.
 *
 * Bytes moved at the least: 4 * G * k * F written to out, 4 * F * sum_g min(n_g, k) read of x, and in the sort mode one key per
 * node — a whole 128-byte line each unless ldkey is 1.
 */
#ifndef TFGX_ROWS3D_H
#define TFGX_ROWS3D_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_ROWS3D_ABI_VERSION 1
int tfgx_rows3d_version(void);   /* the TFGX_ROWS3D_ABI_VERSION the library was built with */

/* The word *flags holds after a sort-mode call: 0, or this bit when a graph had more than TFGX_STATIC_POOL_MAX_GRAPH_NODES
 * nodes.  The value of TFGX_STATIC_POOL_TOO_LONG, so that it can be ORed into counts[3] of a static batch. */
#define TFGX_ROWS3D_TOO_LONG 8

/* ONE launch: one workgroup per graph (ranking, then the copy of its min(n_g, k) rows and the zero fill of the rest), and
 * behind them the workgroups that write -1 to node_slot of the nodes no graph lists and the flag word.
 *   seg_ptr [G + 1]  : the graphs' position offsets, ascending
 *   seg_node [N]     : the node of every position, each node of [0, n_rows) once (then N == n_rows); NULL = the identity
 *                      (then N <= n_rows, and the nodes outside [seg_ptr[0], seg_ptr[G]) are listed by no graph)
 *   x [n_rows, F]    : float32 rows of stride ldx
 *   k >= 1           : slots per graph; G * k fits int32
 *   key, ldkey       : NULL for the plain mode; else key[n * ldkey] ranks node n (the sort column inside x: key = x + c,
 *                      ldkey = ldx)
 *   out [G * k, F]   : rows of stride ldo
 *   slot_node [G * k], node_slot [n_rows] : int32, written
 *   flags [1]        : written in the sort mode (0 or TFGX_ROWS3D_TOO_LONG); in the plain mode it may be NULL and holds 0
 *                      afterwards when it is not
 * Refused: a negative size or one not fitting int32, k < 1, G * k not fitting int32, ldx < F, ldo < F, ldkey < 1 with a key,
 * N > n_rows, seg_node with N != n_rows, a null pointer that the sizes need (flags with a key). */
int tfgx_segment_rows_3d_f32(const int32_t* seg_ptr, const int32_t* seg_node, int64_t G, int64_t N, const float* x, int64_t ldx,
                             int64_t n_rows, int64_t F, int64_t k, const float* key, int64_t ldkey, float* out, int64_t ldo,
                             int32_t* slot_node, int32_t* node_slot, int32_t* flags, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_ROWS3D_H */
