/*
 * tfgx_dense_pool_static — the pooled batch of one fixed-shape DiffPool / MinCutPool level: the diagonal blocks of S^T A S in,
 * a static batch (include/tfgx_collate_static.h) out, at sizes the host knows.  Nothing is read back and nothing is sorted, so a
 * hierarchical classifier with dense pooling over fixed-shape batches is a fixed launch sequence that a hipGraph can replay.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/nn/pool/diff_pool.py:8-105, nn/pool/min_cut_pool.py:127-143 and utils/graph_utils.py:272-284
 * (convert_dense_adj_to_edge: the entries != 0 of the pooled adjacency in row-major order).
 *
 * The parent batch has B slots, graph_mask [B] (one byte per slot, non-zero = live) and counts [4].  P is float32 [B K, K] on
 * leading dimension ldp: rows [g K, (g + 1) K) are slot g's block S_g^T (A S)_g, what tfgx_segment_gram_f32 (tfgx_seggram.h)
 * writes with G = B over the parent's graph_row_ptr[0 .. B].  What the blocks of dead slots hold does not matter.
 *
 * Every live slot becomes exactly K pooled rows and at most K K pooled edges, whatever its graph's size (an empty graph too),
 * so the capacities need no bound: n_cap' = B K + P' rows (the last P' of them the sinks) and e_cap' >= the edges any batch can
 * have (B K K, or B K (K - 1) without the diagonal; the host's arithmetic).  With m_live = K * (live slots) and e_live the
 * number of kept entries, the layout is that of a static batch:
 *   pooled_row_ptr [B + 2] : pooled_row_ptr[g] = K * (live slots before g), then m_live, closed with n_cap'.  A dead slot owns
 *                            no rows;
 *   node_index [n_cap']    : pooled row -> the row g K + c of P (and of the slot-indexed pooled features); rows [m_live, n_cap')
 *                            hold -1;
 *   node_map [B K]         : row g K + c of P -> pooled row, -1 for the rows of a dead slot;
 *   node_graph_index [n_cap'] : the slot of a live pooled row, B for a dead one;
 *   edges [0, e_live)      : the entries of the live slots' blocks with P[g K + c1, c2] != 0.0f (C's comparison: -0.0 is no
 *                            edge, a NaN is one), without c1 == c2 when drop_diagonal, in slot order and row-major order inside
 *                            a slot: row = pooled_row_ptr[g] + c1, col = pooled_row_ptr[g] + c2,
 *                            edge_src = (g K + c1) K + c2 (the flat position in a P of ldp == K), edge_graph_index = g;
 *   edges [e_live, e_cap') : edge q is a unit self-loop on sink t = (q - e_live) / d: row = col = n_cap' - P' + t,
 *                            edge_src = -1, edge_graph_index = B (the rule of tfgx_collate_static.h);
 *   the two plans          : what tfgx_build_csr_by_dst gives for the emitted [2, e_cap'] list and for its flip.  The list is
 *                            sorted by row, so the plan by row has the identity permutation; the plan by column ranks every
 *                            entry of a slot in column-major order inside the slot's own edge range; dead non-sink rows are
 *                            empty, sink rows have a closed form, the padded tail is the identity — no sort;
 *   counts [4]             : live graphs (the parent's, copied), m_live, e_live, the parent's flags carried on.  This level
 *                            adds no flag of its own: its capacities cannot overflow.
 * No weights are written: the pooled weight of edge q is P at edge_src[q] (1.0f where edge_src[q] < 0), which the caller
 * gathers so that it stays differentiable.
 *
 * Launches: a FIXED sequence of three with no host read between them —
 *   count : one workgroup per slot; the non-zero mask of a row of the block is one wave ballot;
 *   scan  : one workgroup scans the B slots (live slots -> row offsets, kept entries -> edge offsets) and writes counts;
 *   emit  : one workgroup per slot (its rows, its edges, its part of both plans; the block's mask is 64 words of 64 bits in
 *           LDS, by row and by column), then workgroups for the dead and sink rows and for the padded tail.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code with
 * text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.  Zero-size
 * calls succeed.  No float atomics and no global atomics: every output is a pure function of the inputs.  Every index read
 * from device memory is held to its array's bounds before it is used as an address, and every store to the capacities; a load
 * that may be out of range is clamped, not predicated.
 */
#ifndef TFGX_DENSE_POOL_STATIC_H
#define TFGX_DENSE_POOL_STATIC_H

#include "tfgx_collate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_DENSE_POOL_STATIC_ABI_VERSION 1
int tfgx_dense_pool_static_version(void);   /* the TFGX_DENSE_POOL_STATIC_ABI_VERSION the library was built with */

/* The most clusters per graph: TFGX_SEGGRAM_MAX_K of tfgx_seggram.h (a row of a block is one wave ballot). */
#define TFGX_DENSE_POOL_STATIC_MAX_K 64

/* The most slots the one-workgroup scan covers. */
#define TFGX_DENSE_POOL_STATIC_MAX_SLOTS 1048576

typedef struct tfgx_dense_pool_static_args {
    /* the blocks and the parent batch */
    const float* P;                  /* [B K, K] rows on leading dimension ldp (floats) */
    int64_t ldp;
    const uint8_t* graph_mask;       /* [B] */
    const int32_t* parent_counts;    /* [4] */
    int64_t B;
    int64_t K;
    int32_t drop_diagonal;           /* non-zero: entries with c1 == c2 are no edges (MinCutPool) */
    /* the pooled capacities */
    int64_t n_cap_out;               /* pooled rows, the sinks included: at least B K + sinks */
    int64_t e_cap;                   /* pooled edges */
    int64_t sinks;                   /* P' */
    int64_t sink_degree;             /* d */
    /* the outputs */
    int32_t* pooled_row_ptr;         /* [B + 2] */
    int32_t* node_index;             /* [n_cap_out] */
    int32_t* node_graph_index;       /* [n_cap_out] */
    int32_t* node_map;               /* [B K] */
    int32_t* out_row;                /* [e_cap] */
    int32_t* out_col;                /* [e_cap] */
    int32_t* out_edge_src;           /* [e_cap] */
    int32_t* out_edge_graph_index;   /* [e_cap] */
    const tfgx_collate_plan* plan;   /* by row: out_row_ptr [n_cap_out + 1], out_col / out_perm [e_cap]; the ds_* members are not read */
    const tfgx_collate_plan* plan_t; /* by column */
    int32_t* counts;                 /* [4] */
    void* workspace;
    size_t workspace_bytes;          /* at least tfgx_dense_pool_static_workspace_bytes(B) */
} tfgx_dense_pool_static_args;

size_t tfgx_dense_pool_static_workspace_bytes(int64_t B);

/* The pooled batch: three launches (count, scan, emit), see above.  Refused on the host, with the member named: a null member
 * that the sizes need (pooled_row_ptr, counts, parent_counts, both plans with their out_row_ptr and the workspace always), a
 * negative size, a size not fitting int32 (B K K and B K + sinks among them), B > TFGX_DENSE_POOL_STATIC_MAX_SLOTS, K outside
 * [1, TFGX_DENSE_POOL_STATIC_MAX_K], ldp < K, sink_degree < 1, sinks * sink_degree < e_cap, n_cap_out < B K + sinks, a
 * workspace that is too small.  B == 0 with n_cap_out == 0 and e_cap == 0 and no output given launches nothing. */
int tfgx_dense_pool_static(const tfgx_dense_pool_static_args* args, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_DENSE_POOL_STATIC_H */
