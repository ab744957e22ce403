/*
 * tfgx_h16 — 16-bit feature tables (bf16 / fp16 STORAGE, float32 ARITHMETIC) for the segment-reduce path of tfgx.h.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Why: the gather kernel runs at the part's random-line ceiling, so a gathered row costs the 128-byte lines it touches.
 * A row stored in 16 bits touches half of them.  The reference casts its features to float32 itself
 * (tf_geometric/data/graph.py:79-86) and parity with it is stated in float32; this header keeps that: storage is opt-in,
 * every multiply, add, max, divide and epilogue term stays float32 in the order of tfgx_segment_reduce_f32.
 *
 * Contract: a reduce over a 16-bit table returns, BIT FOR BIT, what tfgx_segment_reduce_f32 returns for that table widened
 * to float32 with the same plan structures (spans, row_order, hub lists).  Widening is exact for both types.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, nothing allocated here, asynchronous on `stream`,
 * 0 = ok or a TFGX_ERR_* code with text in tfgx_last_error(), deterministic results).  A 16-bit element is the raw bit
 * pattern of an IEEE binary16 (TFGX_DT_F16) or a bfloat16 (TFGX_DT_BF16: the upper half of a float32).
 */
#ifndef TFGX_H16_H
#define TFGX_H16_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TFGX_DT_F32 = 0, TFGX_DT_BF16 = 1, TFGX_DT_F16 = 2 };

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_H16_ABI_VERSION 1
int tfgx_h16_version(void);        /* the TFGX_H16_ABI_VERSION the library was built with */

/* ---------------------------------------------------------------------------------------------
 * tfgx_segment_reduce_f32 over a 16-bit table.  Stands for the same reference ops:
 * tf.gather(x, col) -> gcn_mapper -> tf.math.unsorted_segment_{sum,mean,max}
 * (tf_geometric/nn/kernel/map_reduce.py:60-70, :15-42) plus the fused epilogue of tfgx_reduce_args.
 *
 *   args->x      : [n_src, ldx] 16-bit elements of x_dtype (TFGX_DT_BF16 or TFGX_DT_F16); ldx counts ELEMENTS.
 *                  Rows are 16-byte aligned: ldx % 8 == 0 and a 16-byte aligned base.  Every lane gathers 16-byte vectors
 *                  of 8 elements, and lanes past F read pad columns, so EVERY row, the last included, must be readable
 *                  over its whole stride of ldx elements (what the columns in [F, ldx) hold does not matter).
 *   args->out    : [n_dst, ldo] float32 when out_dtype == TFGX_DT_F32, else 16-bit elements of out_dtype (ldo counts
 *                  elements of that type).  A 16-bit output is the float32 result rounded to nearest even as the LAST step
 *                  (the whole epilogue stays float32); NaN stays NaN.  Only columns [0, F) of rows [0, n_dst) are written.
 *   honoured     : row_begin / row_end / rp_stride (explicit spans), col, w, n_dst, op, act, accumulate (float32 output),
 *                  self_coef (the destination's own row is read from the 16-bit table), bias, add_x / ld_add (float32),
 *                  mean_count, row_order, wide_blocks (+1: column blocks of 128 elements on wide line-aligned rows; results
 *                  do not depend on it), hub_threshold and the hub lists with hub_scratch ([n_hub_chunks, F] float32: the
 *                  same chunk partials, folded in chunk order — hub rows match the float32 route bit for bit as well).
 *   empty rows   : 0 for TFGX_SUM / TFGX_MEAN, -FLT_MAX for TFGX_MAX (then the epilogue), as tfgx_segment_reduce_f32.
 *   refused      : TFGX_ERR_INVALID_ARG, the message names the member — x_tail / edge_tail / verify (the split layouts),
 *                  track (max aggregation is inference-only here), ldx % 8 != 0 or a misaligned x, accumulate together
 *                  with a 16-bit output, an x_dtype other than BF16 / F16, an out_dtype outside the enum.
 * --------------------------------------------------------------------------------------------- */
int tfgx_segment_reduce_h16(const tfgx_reduce_args* args, int32_t x_dtype, int32_t out_dtype, tfgx_stream_t stream);

/* The kernel symbol tfgx_segment_reduce_h16 would launch for these arguments, as rocprofv3 prints it:
 * "seg_reduce_h16_kernel<DT, G, CH, IS_MAX, WEIGHTED, U>" (DT = x_dtype, G lanes per destination row, CH column chunks per
 * lane, U edges per batch, 0 = default).  Host-only, launches nothing, same argument checks as the launch.  buf (host)
 * receives a NUL-terminated string; when buf_bytes is too small it receives the empty string and the call returns
 * TFGX_ERR_INVALID_ARG; nothing is written past buf_bytes (64 bytes hold every name). */
int tfgx_segment_reduce_h16_describe(const tfgx_reduce_args* args, int32_t x_dtype, int32_t out_dtype, char* buf, size_t buf_bytes);

/* Quantise / widen feature rows: dst[i, j] = convert(src[i, j]) for i < n, j < F; src and dst have independent leading
 * dimensions (in elements of their own type).  float32 -> 16 bits rounds to nearest even (what tensor.to(dtype) does:
 * values past the fp16 range become inf, fp16 subnormals are produced), NaN stays NaN; 16 bits -> float32 is exact.
 * Columns in [F, ld_dst) and rows >= n of dst are NOT written.  16-byte accesses where the alignment allows, any 2- / 4-byte
 * aligned layout otherwise.  Stands for tf.cast (tf_geometric/data/graph.py:79-86 casts features to float32).
 * Refused: negative n / F, a dtype other than BF16 / F16, leading dimensions < F, null pointers with n * F > 0. */
int tfgx_rows_f32_to_h16(const float* src, int64_t ld_src, int64_t n, int64_t F, void* dst, int64_t ld_dst, int32_t dtype,
                         tfgx_stream_t stream);
int tfgx_rows_h16_to_f32(const void* src, int64_t ld_src, int32_t dtype, int64_t n, int64_t F, float* dst, int64_t ld_dst,
                         tfgx_stream_t stream);

/* host: row stride, in ELEMENTS, that keeps a gathered [*, F] 16-bit row on the fewest 128-byte lines.  A multiple of 8,
 * >= F.  Candidates: roundup8(F), the next multiple of 32 and of 64 elements, the next power of two (F <= 64); the one with
 * the fewest lines per row on average wins, ties go to the smaller stride; a power-of-two stride of 512 bytes or more gets
 * 64 elements more (see plan.pow2_row_stride).  100 -> 128 (2.5 -> 2 lines), 47 -> 64, 128 -> 128, 256 -> 320. */
int64_t tfgx_h16_friendly_ld(int64_t F);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_H16_H */
