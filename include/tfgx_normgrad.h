/*
 * tfgx_normgrad — the backward of the GCN normalisation (tfgx_segment_weight_sum_f32 + tfgx_gcn_norm_edges_f32 of tfgx.h):
 * the gradient of the raw edge weights given the gradients of the normalised weights and of the self-loop coefficients.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its version do not change.
 *
 * Reference: tf_geometric/nn/conv/gcn.py:32-130, which TensorFlow differentiates op by op
 * (row_deg_inv_sqrt @ A @ col_deg_inv_sqrt).
 *
 * No float atomics, no data-dependent reduction order: results are bit-identical from run to run.  Nothing is allocated and
 * the host is never synchronised.
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error(), host-side argument checks before any device work, zero sizes succeed without a launch).
 */
#ifndef TFGX_NORMGRAD_H
#define TFGX_NORMGRAD_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_NORMGRAD_ABI_VERSION 1
int tfgx_normgrad_version(void);   /* the TFGX_NORMGRAD_ABI_VERSION the library was built with */

/* The three launches of the backward, as bits of `passes`.  TFGX_NORMGRAD_ALL is the backward; a subset launches those passes
 * alone, on the scratch an earlier call left (what a tool that times one launch asks for). */
#define TFGX_NORMGRAD_ROW_PASS 1
#define TFGX_NORMGRAD_COL_PASS 2
#define TFGX_NORMGRAD_EDGE_PASS 4
#define TFGX_NORMGRAD_ALL 7

/*
 * Notation: edge e sits at CSR position e of the [n_rows, n_cols] plan (row_ptr, col), r_e / c_e are its row and column, w the
 * raw weights in CSR order.  row_deg[v] = sum_{r_e = v} w_e + diag and col_deg[v] = sum_{c_e = v} w_e + diag are the arrays the
 * forward computed (col_deg NULL = the symmetric form and every mode but BOTH: the row degrees serve both sides).
 *   p(d) = d^-1/2, q(d) = 1/d, each 0 where the power is inf or NaN (the forward's rule);
 *   p'(d) = -1/2 p(d)^3, q'(d) = -q(d)^2: ZERO wherever the forward zeroed the factor, and zero where the derivative itself
 *   is not finite — a gradient is never inf or NaN because a node is isolated.
 * Inputs: G[e] = dL/d w_out[e] (CSR order), S[v] = dL/d self_coef[v] (NULL: no self coefficient, or none that carries a
 * gradient).  Output: dw[e] = dL/d w[e] (CSR order); every element is written.
 *
 *   BOTH   A[v] = sum_{r_e = v} G_e w_e p_c[c_e]     B[v] = sum_{c_e = v} G_e w_e p_r[r_e]
 *          add_self_loop && renorm && S:  A[v] += S_v fill p_c[v],  B[v] += S_v fill p_r[v]
 *          col_deg == NULL:  D = (A + B) p'(row_deg)                  dw_e = G_e p_r[r_e] p_c[c_e] + D[r_e]
 *          else:  D_r = A p'(row_deg), D_c = B p'(col_deg)            dw_e = G_e p_r[r_e] p_c[c_e] + D_r[r_e] + D_c[c_e]
 *   LEFT   T[v] = sum_{r_e = v} G_e w_e (+ S_v fill if add_self_loop), D = T q'(row_deg)      dw_e = G_e q(row_deg[r_e]) + D[r_e]
 *   RIGHT  T[v] = sum_{c_e = v} G_e w_e (+ S_v fill if add_self_loop), D = T q'(row_deg)      dw_e = G_e q(row_deg[c_e]) + D[r_e]
 *          (the forward scales column c by the ROW degree of node c, so n_cols <= n_rows and the degree term returns along
 *          the row; a row v >= n_cols has D[v] = 0)
 *
 * Three launches: a row pass over (row_ptr, col) that sums A (or T) and writes the per-edge product t_e = G_e w_e p_r[r_e]
 * (RIGHT: G_e w_e) in CSR order; a column pass over the transposed plan's t_row_ptr[n_cols + 1] that sums t[t2d[j]] — t2d[j]
 * is the CSR position of the edge at transposed position j — into B (LEFT has no column pass: t_row_ptr, t2d, B and t may
 * be NULL); an edge pass that writes dw.  Every sum is taken by eight lanes per row in a fixed order with a fixed shuffle
 * tree; a row (or column) of more than 2048 edges is left to its whole workgroup, again in a fixed order.
 *
 * Scratch from the caller: A[n_rows] (BOTH, LEFT), B[n_cols] (BOTH, RIGHT), t[E] (BOTH, RIGHT), E = row_ptr[n_rows]; their
 * contents on return are unspecified.  add_self_loop with n_rows != n_cols is refused, and so is RIGHT with
 * n_cols > n_rows.  w == NULL (an unweighted edge list) is refused: there is nothing to differentiate.
 * passes: a non-empty subset of TFGX_NORMGRAD_ALL.  n_rows == 0: nothing is done.
 */
int tfgx_gcn_norm_backward_f32(const int32_t* row_ptr /* [n_rows+1] */, const int32_t* col /* [E] */, const float* w /* [E] */,
                               int64_t n_rows, int64_t n_cols,
                               const int32_t* t_row_ptr /* [n_cols+1] */, const int32_t* t2d /* [E] */,
                               const float* row_deg /* [n_rows] */, const float* col_deg /* [n_cols] or NULL */,
                               int32_t norm_mode /* TFGX_NORM_* */, float fill, int32_t add_self_loop, int32_t renorm,
                               const float* G /* [E] */, const float* S /* [n_rows] or NULL */,
                               float* A, float* B, float* t, float* dw /* [E] */, int32_t passes, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_NORMGRAD_H */
