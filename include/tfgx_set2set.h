/*
 * tfgx_set2set — the two hot paths of the Set2Set readout: a fused per-graph attention readout (online softmax, one pass
 * over x) with its backward, and a stateful sequence LSTM (initial state in, every h_t and the last state out) with its
 * backward through time.  Exported from libtfgx.so next to the entry points of tfgx.h and tfgx_lstm.h; neither header
 * nor its version changes.
 *
 * Reference: tf_geometric/nn/pool/set2set.py:21-42 (per iteration: lstm over the [1, G, 2F] query sequence, then
 * gather / multiply / row sum / segment_softmax / multiply / segment sum) and nn/kernel/segment.py:26-33 (the softmax:
 * exp(e - stop_gradient(max)) / (sum + 1e-8)).
 *
 * No float atomics, no data-dependent reduction order: results are bit-identical from run to run.  Nothing is allocated.
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error(), host-side argument checks before any device work, zero sizes succeed without a launch).
 */
#ifndef TFGX_SET2SET_H
#define TFGX_SET2SET_H

#include "tfgx.h"
#include "tfgx_lstm.h"   /* TFGX_LSTM_MAX_UNITS */

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_SET2SET_ABI_VERSION 1
int tfgx_set2set_version(void);   /* the TFGX_SET2SET_ABI_VERSION the library was built with */

/* ---- (a) the per-graph attention readout -------------------------------------------------------------------------------
 * A CSR over graphs: row_ptr [G + 1] and node [N], the node ids grouped by graph (any order inside a graph; the order is
 * the order of summation).  x [N, F] (leading dimension ldx), queries q [G, F]:
 *   e_n = <x_n, q_g>      m_g = max_n e_n      p_n = exp(e_n - m_g)      D_g = sum_n p_n + 1e-8
 *   r_g = sum_n (p_n / D_g) x_n                       (a graph without nodes: r_g = 0, m_g = 0, D_g = 1e-8)
 * One wave owns up to TFGX_SET2SET_CHUNK_ROWS consecutive rows of one graph and keeps the running (m, s, r) in registers.
 * A longer graph is cut into chunks of that many rows, counted from the graph's first row; their partial (m, s, r) go to
 * the caller's workspace and a second, small launch merges them in chunk order.
 * F is in [1, TFGX_SET2SET_MAX_FEATURES]; rows are read 16 bytes at a time when F % 4 == 0, ldx % 4 == 0 and x is
 * 16-byte aligned, and 4 bytes at a time otherwise.
 */
#define TFGX_SET2SET_CHUNK_ROWS 512
#define TFGX_SET2SET_MAX_FEATURES 1024

/* Bytes of `workspace` for either direction: 0 when N <= TFGX_SET2SET_CHUNK_ROWS (no graph can be cut), otherwise
 * 4 * (2 G + ceil(N / TFGX_SET2SET_CHUNK_ROWS) * (F + 2)). */
size_t tfgx_set2set_attend_workspace_bytes(int64_t N, int64_t G, int64_t F);

/* Forward.  r [G, F] (ldr >= F) is written for every graph.  stats [G, 2] = (m_g, D_g), dense, or NULL for inference.
 *   A row_ptr span that is not inside [0, N] or runs backwards is treated as an empty graph, a node id outside [0, N) is
 *   skipped; either ORs 1 into *bad_flag (never an out-of-range load).  bad_flag may be NULL; the caller zeroes it.
 *   G == 0 or F == 0: nothing is done.  N == 0: every graph is empty (r = 0). */
int tfgx_set2set_attend_f32(const int32_t* row_ptr, const int32_t* node, int64_t G, int64_t N,
                            const float* x, int64_t ldx, int64_t F, const float* q, int64_t ldq,
                            float* r, int64_t ldr, float* stats /* [G, 2] or NULL */,
                            void* workspace, size_t workspace_bytes, int32_t* bad_flag /* device int32 or NULL */,
                            tfgx_stream_t stream);

/* Backward of one forward launch (same row_ptr, node, x, q and its r and stats).  d_r [G, F] (ldg >= F) is the gradient of
 * r.  One pass over x: e_n and a_n = exp(e_n - m_g) / D_g are recomputed; with da_n = <d_r_g, x_n>, c_g = <d_r_g, r_g>:
 *   de_n = a_n (da_n - c_g)        d_x_n = a_n d_r_g + de_n q_g        d_q_g = sum_n de_n x_n
 * (exact with the epsilon in D; m is a stop-gradient).  Every node lies in one graph, so a d_x row has one writer; d_q of a
 * graph that was cut is merged from its chunks' partial sums in chunk order.
 *   d_x [N, F] (lddx >= F) or NULL (not wanted).  Rows of d_x that `node` does not name are LEFT UNTOUCHED: a caller whose
 *   node list may skip rows zeroes d_x first.  d_q [G, F] (lddq >= F) is written for every graph.
 *   Invalid spans and node ids are skipped as in the forward.  G == 0 or F == 0: nothing is done. */
int tfgx_set2set_attend_backward_f32(const int32_t* row_ptr, const int32_t* node, int64_t G, int64_t N,
                                     const float* x, int64_t ldx, int64_t F, const float* q, int64_t ldq,
                                     const float* r, int64_t ldr, const float* stats, const float* d_r, int64_t ldg,
                                     float* d_x /* or NULL */, int64_t lddx, float* d_q, int64_t lddq,
                                     void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

/* ---- (b) the stateful sequence LSTM --------------------------------------------------------------------------------------
 * The input projection is hoisted (as in tfgx_lstm.h): P [B * T, 4U] holds x_t @ kernel + bias of (row b, step t) at row
 * b * T + t (leading dimension ldp >= 4U); R [U, 4U] dense, gate blocks i, f, c, o of U columns each.
 *   z_t = P[b, t] + h_{t-1} @ R      i, f, o = sigmoid(z_i, z_f, z_o)   g = tanh(z_c)   c_t = f c_{t-1} + i g   h_t = o tanh(c_t)
 * h_{-1} = h0[b], c_{-1} = c0[b] ([B, U] dense; NULL = zeros).  One workgroup of 4U threads (a thread per gate column) owns
 * one batch row when B == 1 and four otherwise, for all T steps; h_t is staged in LDS.
 * U must be a multiple of 16 in [16, TFGX_LSTM_MAX_UNITS = 256] (the Python side zero-pads other widths, which is exact).
 * R is copied to LDS once per workgroup when tfgx_lstm_sequence_kernel_resident(U) and T >= 2 (a single step would read
 * the copy once), otherwise every step reads it from L2.
 */

/* 1 when R [U, 4U] fits in LDS beside the step's tiles (U <= 96), else 0 (also for a bad U). */
int tfgx_lstm_sequence_kernel_resident(int64_t U);

/* Bytes of the training forward's saved state: 4 * B * U * (5 T + 1) (gates and c of every step, and c0).  Opaque layout. */
size_t tfgx_lstm_sequence_saved_bytes(int64_t B, int64_t T, int64_t U);

/* Forward.  h_seq [B * T, U] dense (h_t of (b, t) at row b * T + t), h_last [B, U], c_last [B, U]: each may be NULL (not
 * wanted).  saved == NULL: inference; otherwise saved_bytes >= tfgx_lstm_sequence_saved_bytes(B, T, U).
 * B == 0, T == 0 or U == 0: nothing is done (with T == 0 the caller's last state is its initial state). */
int tfgx_lstm_sequence_f32(const float* P, int64_t ldp, int64_t B, int64_t T, const float* R, int64_t U,
                           const float* h0 /* or NULL */, const float* c0 /* or NULL */,
                           float* h_seq, float* h_last, float* c_last,
                           void* saved /* NULL: inference */, size_t saved_bytes, tfgx_stream_t stream);

/* Backward through time of one forward launch (same B, T, U, R, h0 and its `saved`).  d_h_seq [B * T, U], d_h_last [B, U],
 * d_c_last [B, U] are the gradients of the three outputs; each may be NULL (no gradient).  One launch that walks
 * t = T-1 .. 0 and writes
 *   d_gates [B * T, 4U]: dz of (b, t) at row b * T + t — this IS dP, no gather
 *   h_prev  [B * T, U]:  h_{t-1} of (b, t) at row b * T + t       (so dR = h_prev^T @ d_gates)
 *   d_h0 [B, U], d_c0 [B, U]: the gradients of the initial state.
 * B == 0, T == 0 or U == 0: nothing is done. */
int tfgx_lstm_sequence_backward_f32(int64_t B, int64_t T, int64_t U, const float* R, const float* h0 /* or NULL */,
                                    const float* d_h_seq, const float* d_h_last, const float* d_c_last,
                                    const void* saved, size_t saved_bytes,
                                    float* d_gates, float* h_prev, float* d_h0, float* d_c0, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_SET2SET_H */
