/*
 * tfgx_nbrblock — minibatch neighbour sampling: sample the neighbours of a LIST of nodes and relabel the sampled
 * neighbourhood into a small block, hop by hop, with work proportional to the batch and never to the graph.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler) and demo/demo_graph_sage.py
 * (num_sampled_neighbors_list = [25, 10]: one sampled block per layer).
 *
 * Two pieces, both O(batch):
 *
 * (a) tfgx_nbrblock_sample_rows — the row-list twin of tfgx_sample_neighbors.  Output row i receives
 *     out_ptr[i + 1] - out_ptr[i] neighbours of NODE rows[i]; the generator is keyed by (seed, rows[i], draw), so with the same
 *     seed, count and replace_when_short, row i is bit for bit the slice tfgx_sample_neighbors writes for row rows[i] of the
 *     whole graph (both are compiled from the same per-row bodies), whatever batch the node is in.
 *
 * (b) an order-stable relabel over a PERSISTENT table int32 [n_nodes] the caller keeps between calls.  An entry is
 *     TFGX_NBRBLOCK_EMPTY or the virtual id of that node in the running call.  tfgx_nbrblock_stamp enters the seeds,
 *     tfgx_nbrblock_relabel gives every sampled id its virtual id — ids not yet in the table are numbered n_known,
 *     n_known + 1, ... in order of their FIRST OCCURRENCE in `cols` — and tfgx_nbrblock_reset empties exactly the entries a
 *     call has written.  No sort: an integer atomicMin of (n_known + position) per sampled id leaves, for a new id, its first
 *     position in the table whatever order the atomics land in (a known id's entry is below n_known and is never lowered);
 *     "I am the first occurrence" flags, one exclusive scan, and two plain-store passes finish it.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument: a null
 * pointer the sizes need, a negative size, a total that does not fit int32.  Zero-size calls succeed and launch nothing.
 * One table serves one stream at a time.
 */
#ifndef TFGX_NBRBLOCK_H
#define TFGX_NBRBLOCK_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_NBRBLOCK_ABI_VERSION 1
int tfgx_nbrblock_version(void);   /* the TFGX_NBRBLOCK_ABI_VERSION the library was built with */

/* An entry of the table that holds no virtual id (what the caller fills the table with once). */
#define TFGX_NBRBLOCK_EMPTY 2147483647

/* Bits of the device words `bad_flag` / `flag` (OR-ed in; the caller zeroes the word). */
#define TFGX_NBRBLOCK_BAD_RANGE 1      /* an id outside [0, n_nodes) — compared, never dereferenced */
#define TFGX_NBRBLOCK_BAD_REPEAT 2     /* stamp: an id that is in the table already (a duplicate seed) */

/* Sample neighbours of the nodes rows[0 .. n_rows).
 *   row_ptr [n_nodes + 1], col / w [row_ptr[n_nodes]]: the graph's CSR by destination (w NULL: all ones).  A node without
 *                in-edges — one that only appears as a neighbour included — has row_ptr[r] == row_ptr[r + 1].
 *   rows [n_rows]: global node ids, any order, repeats allowed.
 *   out_ptr [n_rows + 1]: non-decreasing from 0; row i draws out_ptr[i + 1] - out_ptr[i] neighbours (0 for a node without any).
 *   out_col [out_ptr[n_rows]] global neighbour ids, out_w the same (NULL: not written).
 *   bad_flag: one int32 on the device.  A row id outside [0, n_nodes) is compared first, never used as an index: nothing is
 *             written for that row and TFGX_NBRBLOCK_BAD_RANGE is raised.
 * The rules per row are those of tfgx_sample_neighbors (keep-all, with replacement when replace_when_short and more draws than
 * neighbours, Floyd, selection sampling, a wave per long row).  Two launches, both sized by n_rows. */
int tfgx_nbrblock_sample_rows(const int32_t* row_ptr, const int32_t* col, const float* w /* or NULL */, int64_t n_nodes,
                              const int32_t* rows, int64_t n_rows, const int32_t* out_ptr, int32_t replace_when_short,
                              uint64_t seed, int32_t* out_col, float* out_w /* or NULL */, int32_t* bad_flag,
                              tfgx_stream_t stream);

/* table[ids[j]] = base + j for j in [0, n).  Raises TFGX_NBRBLOCK_BAD_RANGE in *flag for an id outside [0, n_nodes) (nothing
 * is written for it) and TFGX_NBRBLOCK_BAD_REPEAT for an id whose entry is not TFGX_NBRBLOCK_EMPTY (the entry keeps its first
 * value).  base + n must fit int32. */
int tfgx_nbrblock_stamp(int32_t* table, int64_t n_nodes, const int32_t* ids, int64_t n, int64_t base, int32_t* flag,
                        tfgx_stream_t stream);

/* Bytes of scratch tfgx_nbrblock_relabel needs for E sampled ids (two int32 [E] arrays and the scan's own). */
size_t tfgx_nbrblock_relabel_workspace_bytes(int64_t E);

/* out_vcol[p] = the virtual id of cols[p], p in [0, E).  The table holds the n_known ids of node_list[0 .. n_known) (virtual
 * id = position); the ids of `cols` it does not hold are appended to node_list in first-occurrence order and entered into the
 * table; *n_new (one int32 on the device) receives how many.  node_list must have room for n_known + E entries.  An id of
 * `cols` outside [0, n_nodes) is skipped (out_vcol = -1): the sampler never emits one.  n_known + E must fit int32. */
int tfgx_nbrblock_relabel(int32_t* table, int64_t n_nodes, int64_t n_known, const int32_t* cols, int64_t E, int32_t* out_vcol,
                          int32_t* node_list, int32_t* n_new, void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

/* table[node_list[j]] = TFGX_NBRBLOCK_EMPTY for j in [0, n): the entries of one call, nothing else.  Ids outside [0, n_nodes)
 * are skipped. */
int tfgx_nbrblock_reset(int32_t* table, int64_t n_nodes, const int32_t* node_list, int64_t n, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_NBRBLOCK_H */
