/*
 * tfgx_seggram — the segmented transposed product out[g] = S_g^T Y_g of the dense pooling layers (DiffPool, MinCutPool) and
 * its backward.  With a block-diagonal assignment (node n of graph g has clusters [gK, (g + 1)K) only) every product those
 * layers need has this form: Y = A S gives the pooled adjacency, Y = h the pooled features, Y = S the orthogonality term.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its version do not change.
 *
 * Reference: tf_geometric/nn/pool/diff_pool.py:42-48 and nn/pool/min_cut_pool.py:31-89, which build a sparse [N, G K]
 * assignment and go through a dense [N, N] adjacency (cluster_pool.py:32-38).
 *
 * No float atomics, no data-dependent reduction order: results are bit-identical from run to run.  Nothing is allocated.
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error(), host-side argument checks before any device work, zero sizes succeed without a launch).
 */
#ifndef TFGX_SEGGRAM_H
#define TFGX_SEGGRAM_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_SEGGRAM_ABI_VERSION 1
int tfgx_seggram_version(void);   /* the TFGX_SEGGRAM_ABI_VERSION the library was built with */

#define TFGX_SEGGRAM_MAX_K 64
int tfgx_seggram_block(void);     /* nodes per position block, a compile-time constant of the library */

/* ---- forward ---------------------------------------------------------------------------------------------------------------
 *   out[g*K + k, w] = sum over the positions p of [seg_ptr[g], seg_ptr[g + 1]), in that order, of S[n_p, k] * Y[n_p, w]
 *   n_p = seg_node[p], or p itself when seg_node is NULL.
 * The position axis is cut into blocks of B = tfgx_seggram_block() positions at the absolute multiples of B.  One workgroup
 * per block (and per 64 columns of W) stages its rows of S and Y in LDS and walks the block in order, one float32 fma chain
 * per output element and segment.  A segment that lies inside one block is written straight to out; a segment that crosses a
 * block boundary leaves one partial per block it touches in the workspace, and the fold adds each such segment's partials
 * in block order: the first block's partial, then the following partials 64 at a time (counted from the segment's own first
 * block, each full group summed first, by a launch of its own when N allows one), then those left over.  So the order of
 * summation is a function of (seg_ptr, seg_node, B) alone, and no segment is one serial chain: a segment's result does not
 * change when other segments change, as long as its own first position keeps its value modulo B.
 * Every row of out is written, the zero rows of an empty segment included; columns at and beyond W are left alone.
 *   seg_ptr must be non-decreasing.  A span that runs backwards or is not inside [0, N] is treated as empty (zero rows) and
 *   ORs 1 into *bad_flag, and so does a seg_node outside [0, N), whose position is skipped; neither is ever an out-of-range
 *   access.  Where the pointer is not monotone the spans that overlap the damaged ones are unspecified (finite or zero rows,
 *   in range); all others are exact.  bad_flag may be NULL; the caller zeroes it.
 *   K in [1, TFGX_SEGGRAM_MAX_K], 0 <= W <= 2^20, G >= 0, N >= 0; N and G * K fit int32.  G == 0 or W == 0: nothing is done.
 *   workspace: tfgx_segment_gram_workspace_bytes(N, G, K, W) bytes (0 when N fits one block: workspace may then be NULL),
 *   aligned to 16 bytes; a smaller one is TFGX_ERR_WORKSPACE. */
size_t tfgx_segment_gram_workspace_bytes(int64_t N, int64_t G, int64_t K, int64_t W);

int tfgx_segment_gram_f32(const int32_t* seg_ptr /* [G+1] */, const int32_t* seg_node /* [N], or NULL = identity */,
                          int64_t G, int64_t N,
                          const float* S, int64_t lds, int64_t K,
                          const float* Y, int64_t ldy, int64_t W,
                          float* out /* [G*K, W] */, int64_t ldo,
                          int32_t* bad_flag /* device int32 or NULL */,
                          void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

/* ---- backward --------------------------------------------------------------------------------------------------------------
 *   dS[n, k] = sum_w Y[n, w] * dOut[seg(n)*K + k, w]      dY[n, w] = sum_k S[n, k] * dOut[seg(n)*K + k, w]
 * seg(n) = node_seg[n] (any order).  Node-parallel: a workgroup takes a run of nodes and keeps the dOut block of the segment
 * it is in, 64 columns at a time, in LDS; every output row is one chain in index order, independent of every other row.
 * dS or dY may be NULL: that output is not computed (S is read for dY only, Y for dS only).  A node_seg outside
 * [0, G) gives zero rows and ORs 1 into *bad_flag.  Every row of the wanted outputs is written (dS is zero when W == 0).
 *   N == 0, or both outputs NULL: nothing is done. */
int tfgx_segment_gram_backward_f32(const int32_t* node_seg /* [N] */, int64_t N, int64_t G,
                                   const float* S, int64_t lds, int64_t K,
                                   const float* Y, int64_t ldy, int64_t W,
                                   const float* dOut, int64_t ldo,
                                   float* dS /* or NULL */, int64_t ldds,
                                   float* dY /* or NULL */, int64_t lddy,
                                   int32_t* bad_flag, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_SEGGRAM_H */
