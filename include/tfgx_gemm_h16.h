/*
 * tfgx_gemm_h16 — the dense GEMM of tfgx.h (tfgx_gemm_bias_act_cols_ws_f32) and its weight gradient (tfgx_gemm_tn_gated_f32)
 * reading their first operand from a 16-bit feature table (tfgx_h16.h: bf16 / fp16 STORAGE, float32 ARITHMETIC).  Exported
 * from libtfgx.so next to the entry points of tfgx.h, tfgx_h16.h and tfgx_fused_h16.h; those headers and their version
 * constants do not change.
 *
 * Why: the GEMM-first layers (GCN with units <= F, GAT's Q / K / V projections, the self half and the narrow route of mean /
 * sum GraphSAGE) project the widest tables there are — raw input features, 602 or 1433 columns into 16 .. 256 — and on the
 * narrow outputs those products stream A and do little else.  A table stored in 16 bits is half the bytes to stream and
 * half the memory to hold; widening it first writes and re-reads a float32 copy of the whole table.
 *
 * Contract: every kernel loads the 16-bit elements, widens them in registers (exact for both types) and feeds the float32
 * MFMAs in the float32 kernel's lane -> k mapping and step order.  B, bias, C, G, gate, dW and db stay float32.
 *   - tfgx_gemm_bias_act_cols_ws_h16 writes, BIT FOR BIT, what tfgx_gemm_bias_act_cols_ws_f32 writes for the table widened
 *     into a dense float32 matrix (lda = K on a 16-byte aligned base) with the same B, bias, act, act_cols, ldc, M, K, N and
 *     the same workspace size.  It takes the ROUTE that float32 call takes (kernel, tile, split-K, slices, remainder): the
 *     routes are decided for lda = K on an aligned base, whatever stride the table itself has.
 *   - tfgx_gemm_tn_gated_h16 writes, bit for bit, the dW and db of tfgx_gemm_tn_gated_f32 on that matrix.
 *   - What the padding columns [K, lda) of the table hold never reaches a result: no element at k >= K is multiplied.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, nothing allocated here, asynchronous on `stream`,
 * 0 = ok or a TFGX_ERR_* code with text in tfgx_last_error(), deterministic results).  Workspace sizes are those of
 * tfgx_gemm_workspace_bytes and tfgx_gemm_tn_workspace_bytes.
 */
#ifndef TFGX_GEMM_H16_H
#define TFGX_GEMM_H16_H

#include "tfgx_h16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_GEMM_H16_ABI_VERSION 1
int tfgx_gemm_h16_version(void);        /* the TFGX_GEMM_H16_ABI_VERSION the library was built with */

/* C[M, N] = act(A[M, K] @ B[K, N] + bias), activation on columns [0, act_cols): tfgx_gemm_bias_act_cols_ws_f32 with
 *   A        : [M, lda] 16-bit elements of a_dtype (TFGX_DT_BF16 | TFGX_DT_F16); lda counts ELEMENTS, lda % 8 == 0, lda >= K,
 *              16-byte aligned base; every row readable over its whole stride.
 *   the rest : as tfgx_gemm_bias_act_cols_ws_f32 (float32 B, bias, C; workspace NULL or tfgx_gemm_workspace_bytes(M, K, N)).
 *   refused  : TFGX_ERR_INVALID_ARG on the host, before any device work, the message names the member — an a_dtype other
 *              than BF16 / F16, lda % 8 != 0, a misaligned A, lda < K, and everything the float32 entry refuses. */
int tfgx_gemm_bias_act_cols_ws_h16(const void* A, int32_t a_dtype, int64_t lda, const float* B, int64_t ldb,
                                   const float* bias, int32_t act, int64_t act_cols, float* C, int64_t ldc, int64_t M,
                                   int64_t K, int64_t N, void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

/* The route tfgx_gemm_bias_act_cols_ws_h16 takes for these arguments: "bf16 " or "f16 " followed by exactly the text
 * tfgx_gemm_describe returns for the float32 call on the widened dense matrix.  Host-only, launches nothing, the argument
 * checks of the launch; pointers are looked at for alignment and null-ness only.  buf (host) receives a NUL-terminated
 * string; when buf_bytes is too small, or on a refusal, it receives the empty string and the call returns
 * TFGX_ERR_INVALID_ARG; nothing is written past buf_bytes (160 bytes hold every route). */
int tfgx_gemm_h16_describe(const void* A, int32_t a_dtype, int64_t lda, const float* B, int64_t ldb, const float* bias,
                           int32_t act, int64_t act_cols, const float* C, int64_t ldc, int64_t M, int64_t K, int64_t N,
                           void* workspace, size_t workspace_bytes, char* buf, size_t buf_bytes);

/* dW[Ka, N] = X[M, Ka]^T @ G[M, N] (G counted only where gate > 0 when gate != NULL), db[N] = column sums of that G when
 * db != NULL: tfgx_gemm_tn_gated_f32 with
 *   X        : [M, ldx] 16-bit elements of x_dtype under the rules of A above (ldx % 8 == 0, ldx >= Ka, aligned base).
 *   the rest : as tfgx_gemm_tn_gated_f32 (workspace: tfgx_gemm_tn_workspace_bytes(M, Ka, N, db != NULL)).
 *   M == 0   : dW (and db) are zeroed.
 *   refused  : as above for X / x_dtype / ldx, everything the float32 entry refuses, and TFGX_TN_DIRECT=0 in the environment
 *              (the LDS-staged kernel kept for A/B runs reads float32 only). */
int tfgx_gemm_tn_gated_h16(const void* X, int32_t x_dtype, int64_t ldx, const float* G, int64_t ldg, const float* gate,
                           int64_t ld_gate, int64_t M, int64_t Ka, int64_t N, float* dW, int64_t ldw, float* db,
                           void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_GEMM_H16_H */
