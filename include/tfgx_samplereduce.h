/*
 * tfgx_samplereduce — the input hop of minibatch GraphSAGE in one launch: for every listed node, draw its neighbours and reduce
 * their feature rows straight out of the global table.  No edge list, no virtual ids, no gathered copy of the table.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler) and demo/demo_graph_sage.py (mean / sum
 * GraphSAGE are linear in the neighbour reduction, and the outermost hop's ids are consumed by that reduction alone).
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.
 */
#ifndef TFGX_SAMPLEREDUCE_H
#define TFGX_SAMPLEREDUCE_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_SAMPLEREDUCE_ABI_VERSION 1
int tfgx_samplereduce_version(void);   /* the TFGX_SAMPLEREDUCE_ABI_VERSION the library was built with */

/* The largest k: a wave keeps the drawn lists of a tile of rows in 8 KiB of LDS (1024 (id, weight) pairs), a workgroup of
 * four waves 32 KiB — five workgroups, 20 waves, per CU — and a tile holds at least four rows. */
#define TFGX_SAMPLEREDUCE_MAX_DRAWS 256

/* The bit of the device word `bad_flag` (OR-ed in; the caller zeroes the word): a row id outside [0, n_nodes) — compared,
 * never dereferenced.  The value of TFGX_NBRBLOCK_BAD_RANGE (tfgx_nbrblock.h). */
#define TFGX_SAMPLEREDUCE_BAD_RANGE 1

/* out[i, :F] = reduce_j w_j * x[c_j, :F] over the m neighbours (c_j, w_j) drawn for node rows[i], i in [0, n_rows).
 *   row_ptr [n_nodes + 1], col / w [row_ptr[n_nodes]]: the graph's CSR by destination (w NULL: all ones).
 *   rows [n_rows]: global node ids, any order, repeats allowed.
 *   k, replace_when_short: node r with d neighbours draws m = min(d, k) of them, or m = k when replace_when_short and d > 0
 *                — the counts of tfgx_nbrblock_sample_rows' callers.  The draw is keyed by (seed, r): ids and weights are
 *                bit for bit what tfgx_nbrblock_sample_rows writes for that row with the same seed.  0 <= k <=
 *                TFGX_SAMPLEREDUCE_MAX_DRAWS.
 *   x [>= n_nodes rows, ldx floats apart], F columns read; out [n_rows rows, ldo floats apart], F columns written.
 *   op: TFGX_SUM, or TFGX_MEAN (the sum divided by max(m, 1)).  A row without draws is zeros.
 *   out_count [n_rows] or NULL: m per row.
 *   bad_flag: one int32 on the device.  A row id outside [0, n_nodes) writes nothing for its row and raises
 *             TFGX_SAMPLEREDUCE_BAD_RANGE.
 * float32 accumulation in draw order, no float atomics: a row's bits depend on (r, k, replace_when_short, seed, x, w) only.
 * One launch.  n_rows == 0 succeeds and launches nothing. */
int tfgx_samplereduce_f32(const int32_t* row_ptr, const int32_t* col, const float* w /* or NULL */, int64_t n_nodes,
                          const int32_t* rows, int64_t n_rows, int32_t k, int32_t replace_when_short, uint64_t seed,
                          const float* x, int64_t ldx, int64_t F, int32_t op /* TFGX_SUM | TFGX_MEAN */,
                          float* out, int64_t ldo, int32_t* out_count /* [n_rows] or NULL */,
                          int32_t* bad_flag, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_SAMPLEREDUCE_H */
