/*
 * tfgx_fused_h16 — the fused aggregate -> project launch of tfgx.h (tfgx_aggregate_gemm_f32) over a 16-bit feature table
 * (tfgx_h16.h: bf16 / fp16 STORAGE, float32 ARITHMETIC).  Exported from libtfgx.so next to the entry points of tfgx.h and
 * tfgx_h16.h; those headers and their version constants do not change.
 *
 * Why: the aggregate-then-project layers (GCN with units > F, the neighbour half of mean / sum GraphSAGE) are bound by the
 * gather.  A 16-bit table halves the 128-byte lines a gathered row touches; the fused launch keeps the [n_dst, F] aggregate
 * out of HBM.  This header gives a layer both at once.
 *
 * Contract: the call returns, BIT FOR BIT, what tfgx_aggregate_gemm_f32 returns for the table widened to float32 with the
 * same plan structures (row_order, hub lists, hub_order_slot) — for C and for the side output args->out.  Widening is exact
 * for both types; every multiply, add, divide and the MFMA k order are those of the float32 kernel.  Run-to-run identical.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, nothing allocated here, asynchronous on `stream`,
 * 0 = ok or a TFGX_ERR_* code with text in tfgx_last_error()).
 */
#ifndef TFGX_FUSED_H16_H
#define TFGX_FUSED_H16_H

#include "tfgx_h16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_FUSED_H16_ABI_VERSION 1
int tfgx_fused_h16_version(void);        /* the TFGX_FUSED_H16_ABI_VERSION the library was built with */

/* C[n_dst, N] = act( reduce(args) @ B[F, N] + bias ), reduce(args) being what tfgx_segment_reduce_h16 writes as float32 for
 * `args` (op TFGX_SUM | TFGX_MEAN; w, self_coef, mean_count, row_order honoured; args->act / args->bias are NOT used).
 *
 *   envelope   : tfgx_aggregate_gemm_fits(F, N) == 1 (tfgx.h): F % 4 == 0, 4 <= F <= 128, N <= 256.
 *   args->x    : [n_src, ldx] 16-bit elements of x_dtype (TFGX_DT_BF16 | TFGX_DT_F16) under tfgx_h16.h's rules: ldx % 8 == 0,
 *                16-byte aligned base, ldx >= roundup8(F), EVERY row readable over its whole stride of ldx elements (lanes past
 *                F read pad columns and discard them; what the pad columns hold never reaches an output).
 *   B, bias, C : float32, as tfgx_aggregate_gemm_f32 (ldb >= N, ldc >= N; C may be a column block of a wider buffer).
 *   args->out  : NULL, or float32 [n_dst, ldo] (ldo >= F, ldo % 4 == 0, 16-byte aligned) that ALSO receives the aggregate itself
 *                (the training forward: the weight gradient needs it).  Only columns [0, F) are written.
 *   hub lists  : honoured as by tfgx_aggregate_gemm_f32; the chunk partials are written to hub_scratch ([n_hub_chunks, F]
 *                float32, 16-byte aligned) by a launch of tfgx_segment_reduce_h16 first and folded in chunk order.
 *   refused    : TFGX_ERR_INVALID_ARG, the message names the member — x_tail / edge_tail / verify (the split layouts), track,
 *                accumulate, add_x, explicit spans (anything but row_end == row_begin + 1, rp_stride == 1), op == TFGX_MAX, an
 *                x_dtype other than BF16 / F16, a misaligned x, an ldx that is not a multiple of 8.
 *   n_dst == 0 : TFGX_OK, nothing launched. */
int tfgx_aggregate_gemm_h16(const tfgx_reduce_args* args /* host */, int32_t x_dtype, const float* B, int64_t ldb,
                            const float* bias, int32_t act, float* C, int64_t ldc, int64_t N, tfgx_stream_t stream);

/* The kernel symbol tfgx_aggregate_gemm_h16 would launch, as rocprofv3 prints it: "agg_gemm_h16_kernel<DT, G, WEIGHTED>"
 * (DT = x_dtype; G lanes per destination row: 8 for F <= 64, else 16 — never below 8, the tile's units must cover its eight
 * consumer jobs).  Host-only, launches nothing, the argument checks of the launch (all that do not need B / C).  buf (host)
 * receives a NUL-terminated string; when buf_bytes is too small, or on a refusal, it receives the empty string and the call
 * returns TFGX_ERR_INVALID_ARG; nothing is written past buf_bytes (48 bytes hold every name). */
int tfgx_aggregate_gemm_h16_describe(const tfgx_reduce_args* args /* host */, int32_t x_dtype, int64_t N, char* buf,
                                     size_t buf_bytes);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_FUSED_H16_H */
