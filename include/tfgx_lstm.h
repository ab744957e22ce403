/*
 * tfgx_lstm — the LSTM neighbourhood aggregator of GraphSAGE: a fused gather -> recurrence kernel and its BPTT.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/nn/conv/graph_sage.py:290-356 (lstm_graph_sage: a dense [N, T, F] gather of the padded neighbour
 * matrix, a Keras LSTM over it, the mean of h_t over all T steps).
 *
 * Decomposition: the input projection is hoisted out of the recurrence.  The caller computes P = x @ kernel + bias
 * ([n_src, 4U], one GEMM) and hands the kernel P, the pad row p_pad (= bias: the projection of a zero input) and the
 * recurrent kernel R [U, 4U] (row-major, leading dimension 4U, gate blocks i, f, c, o of U columns each).
 * Row i of a destination CSR (row_ptr [n_dst + 1], col) runs T steps:
 *   z_t = (t < deg(i) ? P[col[row_ptr[i] + t]] : p_pad) + h_{t-1} @ R,     h_0 = c_0 = 0
 *   i, f, o = sigmoid(z_i, z_f, z_o),  g = tanh(z_c),  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
 *   out_mean[i] = (sum_t h_t) / T            (pad steps included: the reference's LSTM is not masked)
 * h @ R runs on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: a k-ordered fmaf chain per element).
 *
 * U must be a multiple of 16 in [16, 256] (the Python side zero-pads other widths, which is exact).
 * R is kept in LDS for the whole launch when tfgx_lstm_recurrent_kernel_resident(U, backward) says so, otherwise every
 * step streams it from L2 into the MFMA operand registers.
 *
 * No float atomics, no data-dependent reduction order: results are bit-identical from run to run.  Nothing is allocated.
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code with
 * text in tfgx_last_error(), host-side argument checks before any device work, zero sizes succeed without a kernel launch).
 */
#ifndef TFGX_LSTM_H
#define TFGX_LSTM_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_LSTM_ABI_VERSION 1
int tfgx_lstm_version(void);   /* the TFGX_LSTM_ABI_VERSION the library was built with */

#define TFGX_LSTM_MAX_UNITS 256
#define TFGX_LSTM_TILE_ROWS 32   /* destination rows one workgroup owns for all T steps */

/* 1 when R stays in LDS for the whole launch at this U (backward == 0: forward, 1: backward), else 0 (also for a bad U). */
int tfgx_lstm_recurrent_kernel_resident(int64_t U, int32_t backward);

/* Bytes of the training forward's per-step state for (n_dst, T, U): 20 U bytes per (row, step).  The layout is opaque. */
size_t tfgx_lstm_aggregate_saved_bytes(int64_t n_dst, int64_t T, int64_t U);

/* Workgroup tiles of a launch over n_dst rows = rows of d_pad_partial: ceil(n_dst / TFGX_LSTM_TILE_ROWS). */
int64_t tfgx_lstm_aggregate_tiles(int64_t n_dst);

/* Forward.  P [n_src, 4U] with leading dimension ldp >= 4U, p_pad [4U], R [U, 4U] dense, out_mean [n_dst, U] with ldo >= U.
 *   saved == NULL: inference.  Otherwise saved_bytes >= tfgx_lstm_aggregate_saved_bytes(n_dst, T, U) and the per-step state of
 *   every row is stored for tfgx_lstm_aggregate_backward_f32.
 *   A row with deg(i) > T is truncated to its first T neighbours and ORs 1 into *bad_flag; a col outside [0, n_src) is
 *   treated as a pad step and ORs 1 into *bad_flag (never an out-of-range load).  bad_flag may be NULL; the caller zeroes it.
 *   n_dst == 0 or U == 0: nothing is done.  T == 0: out_mean is zeroed (the mean over no steps is defined as 0 here). */
int tfgx_lstm_aggregate_f32(const int32_t* row_ptr, const int32_t* col, int64_t n_dst, int64_t n_src, int64_t T,
                            const float* P, int64_t ldp, const float* p_pad /* [4U] */, const float* R /* [U, 4U] */, int64_t U,
                            float* out_mean /* [n_dst, U] */, int64_t ldo,
                            void* saved /* NULL: inference */, size_t saved_bytes,
                            int32_t* bad_flag /* device int32 or NULL */, tfgx_stream_t stream);

/* Backward through time of one forward launch (same row_ptr, n_dst, T, U, R and its `saved`).  d_mean [n_dst, U] (ldd >= U) is
 * the gradient of out_mean.  One launch; per tile it walks t = T-1 .. 0 with dh_t = d_mean / T + dz_{t+1} @ R^T (MFMA) and writes
 *   d_gates [n_dst * T, 4U]: dz of (row i, step t) at row i * T + t    (the gradient of the gathered P row / of p_pad)
 *   h_prev  [n_dst * T, U]:  h_{t-1} of (row i, step t) at row i * T + t     (so dR = h_prev^T @ d_gates)
 *   d_pad_partial [tfgx_lstm_aggregate_tiles(n_dst), 4U]: each tile's sum of dz over its pad positions (t >= deg(i)), added in
 *   a fixed order with a compensated (Kahan) running sum per lane; d p_pad is the column sum of this matrix.
 * A forward that raised bad_flag has no defined backward.  n_dst == 0, T == 0 or U == 0: nothing is done. */
int tfgx_lstm_aggregate_backward_f32(const int32_t* row_ptr, int64_t n_dst, int64_t T, int64_t U, const float* R,
                                     const float* d_mean, int64_t ldd, const void* saved, size_t saved_bytes,
                                     float* d_gates, float* h_prev, float* d_pad_partial, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_LSTM_H */
