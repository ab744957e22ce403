/*
 * tfgx_dropedge — DropEdge: device-side edge dropout that hands on sort-free CSR plans.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/nn/sampling/drop_edge.py:6-52 (tf.nn.dropout of a vector of ones -> tf.boolean_mask ->
 * tf.gather of edge_index and of every edge attribute).  A DropEdge training step draws a new edge list every step, so
 * every step would pay for a new plan (a radix sort) and, for the backward pass, for the transposed plan (a second one).
 *
 * Keep rule: edge e (its ORIGINAL id, the position in the input list) survives iff tfgx_dropout_keep(seed, e, rate) != 0
 * (tfgx.h) — a pure function of (seed, e).  rate == 0 keeps everything, rate == 1 keeps nothing.  Because the rule does
 * not depend on where an edge is stored, the edge-order list, the by-destination CSR and the by-source CSR are each
 * compacted on their own, in their own order, and still describe the same graph:
 *   - an order-stable compaction of the PARENT plan's (col, perm) arrays IS the CSR order tfgx_build_csr_by_dst gives the
 *     dropped list (that build is a stable sort by destination, and the new id of a kept edge grows with its old id);
 *   - new row_ptr[r] = number of kept CSR positions below the parent's row_ptr[r];
 *   - new perm[q] = number of kept edge ids below the old id: one 16-byte read of a table that holds, per 64 edges, the
 *     keep bits and the kept count before them (E / 4 bytes, cache-resident where an E-sized rank array is not).
 * No row is walked, so rows shorter and longer than a wave take the same fixed-order path.  No sort, no atomics on data
 * (one integer atomicOr raises the bad-index flag), nothing allocated here, results depend on (seed, rate, input) only.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream` except where stated,
 * 0 = ok or a TFGX_ERR_* code with text in tfgx_last_error()).
 */
#ifndef TFGX_DROPEDGE_H
#define TFGX_DROPEDGE_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_DROPEDGE_ABI_VERSION 1
int tfgx_dropedge_version(void);   /* the TFGX_DROPEDGE_ABI_VERSION the library was built with */

/* One CSR plan of the INPUT edge list (tfgx_build_csr_by_dst layout) and where the dropped list's plan goes.
 *   by destination: parent_* = build(row, col) as an [n_dst, n_src] operator, n_rows = n_dst;
 *   by source     : parent_* = build(col, row) as an [n_src, n_dst] operator (the transposed plan), n_rows = n_src.
 * out_row_ptr [n_rows + 1], out_col [n_out], out_perm [n_out].  The outputs are BIT-IDENTICAL to tfgx_build_csr_by_dst of
 * the emitted list (of its flip, for the by-source plan).  A parent plan that belongs to another edge list is the caller's
 * mistake; it never makes the library write past n_out entries or read outside its workspace. */
typedef struct tfgx_drop_edge_plan {
    const int32_t* parent_row_ptr;   /* [n_rows + 1] */
    const int32_t* parent_col;       /* [E] */
    const int32_t* parent_perm;      /* [E] CSR position -> original edge id */
    int32_t* out_row_ptr;
    int32_t* out_col;
    int32_t* out_perm;
} tfgx_drop_edge_plan;

/* host: bytes of workspace both calls below need (the SAME buffer goes to count and then to emit, untouched between).
 * with_plan / with_plan_t: emit will be given a by-destination / by-source tfgx_drop_edge_plan.  0 for negative sizes. */
size_t tfgx_drop_edge_workspace_bytes(int64_t E, int64_t n_dst, int64_t n_src, int32_t with_plan, int32_t with_plan_t);

/* Pass 1: per-tile kept counts, one scan, and ONE device -> host read of {output edge count, bad-index flag}: the only
 * synchronisation of the operator.
 *   row, col [E]      : the edge list (row = destination in [0, n_dst), col = source in [0, n_src)).
 *   rate              : in [0, 1]; anything else (NaN included) -> TFGX_ERR_INVALID_ARG before any device work.
 *   force_undirected  : 0: every edge is a candidate.  1: the candidates are the edges with row < col, each keyed on its
 *                       own id; needs n_dst == n_src.
 *   n_out (host)      : number of edges emit will write: the kept count, or TWICE the kept candidates when force_undirected.
 * An endpoint outside its range -> TFGX_ERR_INDEX (nothing is emitted).  E == 0 succeeds with *n_out = 0. */
int tfgx_drop_edge_count(const int32_t* row, const int32_t* col, int64_t E, int64_t n_dst, int64_t n_src, float rate,
                         uint64_t seed, int32_t force_undirected, int64_t* n_out, void* workspace, size_t workspace_bytes,
                         tfgx_stream_t stream);

/* Pass 2 (asynchronous): same row / col / E / n_dst / n_src / rate / seed / force_undirected / workspace as the count call,
 * n_out as it returned.
 *   out_row, out_col, out_edge_id [n_out]: the kept edges in their original order and the original id of each.
 *     force_undirected: [kept candidates in input order | the same edges flipped]; out_edge_id repeats the candidate's id
 *     for its mirror (the reference's index = concat([index, index])).
 *   plan / plan_t     : NULL, or the by-destination / by-source plan of the input list and the outputs for the dropped
 *                       list's; the workspace must have been sized for them.  Refused together with force_undirected. */
int tfgx_drop_edge_emit(const int32_t* row, const int32_t* col, int64_t E, int64_t n_dst, int64_t n_src, float rate,
                        uint64_t seed, int32_t force_undirected, int64_t n_out, int32_t* out_row, int32_t* out_col,
                        int32_t* out_edge_id, const tfgx_drop_edge_plan* plan, const tfgx_drop_edge_plan* plan_t,
                        void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_DROPEDGE_H */
