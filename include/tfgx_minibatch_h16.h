/*
 * tfgx_minibatch_h16 — the minibatch route (tfgx_samplereduce.h, tfgx_nbrstatic.h) over a 16-BIT feature table (bf16 / fp16
 * STORAGE, float32 ARITHMETIC: tfgx_h16.h): the fused input hop in its two forms, and the gather that widens.
 * Exported from libtfgx.so next to the entry points of tfgx.h; no other header and no other version changes.
 *
 * Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler), demo/demo_graph_sage.py; the reference casts its
 * features to float32 itself (tf_geometric/data/graph.py:79-86) and parity with it is stated in float32.
 *
 * Contract: every entry point returns, BIT FOR BIT, what its float32 twin returns for the table widened to float32 with the same
 * other arguments — out, out_count and the flag:
 *     tfgx_sample_reduce_h16          <->  tfgx_samplereduce_f32
 *     tfgx_nbr_static_input_hop_h16   <->  tfgx_nbrstatic_input_hop_f32
 *     tfgx_gather_rows_h16_f32        <->  tfgx_nbrstatic_gather_rows_f32
 * Widening is exact for both types, and per column the arithmetic is the float32 kernel's: fmaf(w_j, x, acc) in draw order, then
 * / float(max(m, 1)) for the mean.
 *
 * The table (conventions of tfgx_h16.h): `x` holds raw 16-bit elements of x_dtype (TFGX_DT_BF16 or TFGX_DT_F16), rows ldx
 * ELEMENTS apart, ldx % 8 == 0 and a 16-byte aligned base.  A lane reads 16-byte vectors of 8 elements, the pad columns of the
 * last one included, so EVERY row, the last included, must be readable over its whole stride; what the columns in [F, ldx) hold
 * does not matter (they are loaded, accumulated and never stored).  Only columns [0, F) of `out` are written.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code with
 * text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument: an x_dtype other
 * than BF16 / F16, ldx % 8 != 0, a misaligned x, ldx < F, and every refusal of the float32 twin.
 */
#ifndef TFGX_MINIBATCH_H16_H
#define TFGX_MINIBATCH_H16_H

#include "tfgx_h16.h"
#include "tfgx_samplereduce.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_MINIBATCH_H16_ABI_VERSION 1
int tfgx_minibatch_h16_version(void);   /* the TFGX_MINIBATCH_H16_ABI_VERSION the library was built with */

/* tfgx_samplereduce_f32 over a 16-bit table: out[i, :F] = reduce_j w_j * widen(x[c_j, :F]) over the m neighbours (c_j, w_j) drawn
 * for node rows[i].  Every limit, flag bit and draw is that entry point's: 0 <= k <= TFGX_SAMPLEREDUCE_MAX_DRAWS, a row id outside
 * [0, n_nodes) is compared, never dereferenced, writes nothing for its row and raises TFGX_SAMPLEREDUCE_BAD_RANGE in *bad_flag.
 * out is float32 [n_rows rows, ldo floats apart].  One launch; n_rows == 0 succeeds and launches nothing. */
int tfgx_sample_reduce_h16(const int32_t* row_ptr, const int32_t* col, const float* w /* or NULL */, int64_t n_nodes,
                           const int32_t* rows, int64_t n_rows, int32_t k, int32_t replace_when_short, uint64_t seed,
                           const void* x, int64_t ldx, int64_t F, int32_t x_dtype /* TFGX_DT_BF16 | TFGX_DT_F16 */,
                           int32_t op /* TFGX_SUM | TFGX_MEAN */, float* out, int64_t ldo,
                           int32_t* out_count /* [n_rows] or NULL */, int32_t* bad_flag, tfgx_stream_t stream);

/* tfgx_nbrstatic_input_hop_f32 over a 16-bit table: the same launch with the seed read from the device (hop `hop`'s mix of *seed).
 * A dead row (node[i] < 0) gives a row of zeros and count 0 and raises no flag. */
int tfgx_nbr_static_input_hop_h16(const int32_t* row_ptr, const int32_t* col, const float* w /* or NULL */, int64_t n_nodes,
                                  const int32_t* node, int64_t n_rows, int32_t k, int32_t replace_when_short,
                                  const uint64_t* seed, int32_t hop, const void* x, int64_t ldx, int64_t F,
                                  int32_t x_dtype /* TFGX_DT_BF16 | TFGX_DT_F16 */, int32_t op /* TFGX_SUM | TFGX_MEAN */,
                                  float* out, int64_t ldo, int32_t* out_count /* [n_rows] or NULL */, int32_t* bad_flag,
                                  tfgx_stream_t stream);

/* out[i, :F] = widen(x[idx[i], :F]) for idx[i] >= 0 and zeros for idx[i] < 0, i in [0, M); out float32 [M rows, ldo floats apart].
 * A lane takes one 16-byte vector of 8 elements, widens it and stores float32: 16-byte stores where out allows them (ldo % 4 == 0
 * and a 16-byte aligned base), one store per column otherwise; the last vector is masked to F.  A dead row loads row 0 and drops
 * the value with a select: no load is predicated (so x holds a row whenever M > 0).  An id >= the table's rows is the caller's
 * error (not checked).  Serves the gather of both minibatch classes.  M == 0 succeeds and launches nothing. */
int tfgx_gather_rows_h16_f32(const void* x, int64_t ldx, int32_t x_dtype /* TFGX_DT_BF16 | TFGX_DT_F16 */, const int32_t* idx,
                             int64_t M, int64_t F, float* out, int64_t ldo, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_MINIBATCH_H16_H */
