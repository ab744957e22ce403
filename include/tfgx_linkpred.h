/*
 * tfgx_linkpred — link prediction: a per-edge dot-product decoder and device-side negative sampling.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/utils/graph_utils.py:369-412 (negative_sampling: a dense [N, N] float64 matrix), :415-452
 * (negative_sampling_with_start_node: a Python `while True` per sample) and demo/demo_gae.py (the decoder
 * logit[e] = <z[row[e]], z[col[e]]>, two gathers and a reduce_sum).
 *
 * Draw rule: candidate pair (u, v) of (seed, slot, attempt) is tfgx_negative_draw below, a pure function built on the
 * library's counter-based mixer (the one behind tfgx_dropout_keep), so the host restates every sample: slot s of a call
 * tries attempts 0, 1, ... of slot_base + s and keeps the first candidate that passes the filter.  The samplers are
 * rejection samplers over a SORTED ADJACENCY: adj_ptr [num_nodes + 1], adj_col [adj_ptr[num_nodes]], the columns of a row
 * STRICTLY ASCENDING and inside [0, num_nodes), no (i, i) entries; a membership test is a binary search inside one row.
 * The adjacency is the caller's to get right: a row_ptr that is not monotone or exceeds the array is not detected.
 *
 * No float atomics and no data-dependent reduction order anywhere: results are pure functions of the inputs.  The only
 * atomics are integer ones on the caller's flag / counter words.  Nothing is allocated here.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_*
 * code with text in tfgx_last_error(), host-side argument checks before any device work).  NONE of the calls below
 * synchronises: what the device finds out (a bad endpoint, an exhausted slot) is left in a device word the caller reads.
 */
#ifndef TFGX_LINKPRED_H
#define TFGX_LINKPRED_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_LINKPRED_ABI_VERSION 1
int tfgx_linkpred_version(void);   /* the TFGX_LINKPRED_ABI_VERSION the library was built with */

/* Bit 31 of *n_failed: a start node of tfgx_negative_sample_from was outside [0, num_nodes) (the caller reports
 * TFGX_ERR_INDEX).  Bits 0-30 count the slots that exhausted max_attempts. */
#define TFGX_NEGATIVE_BAD_START ((int32_t)0x80000000)

/* out[e] = sum_f a[row[e], f] * b[col[e], f] for e in [0, E), in the caller's edge order; a == b is allowed.
 *   a [n_a, F] with leading dimension lda >= F, b [n_b, F] with ldb >= F.  16-byte loads when a, b are 16-byte aligned
 *   and lda, ldb, F are multiples of 4; a 4-byte-load path otherwise.  Each path sums in one fixed order (a chain per
 *   lane over the 64-column chunks, then a fixed 16-lane tree): bit-identical from run to run.
 *   An endpoint outside [0, n_a) / [0, n_b) writes out[e] = 0 and ORs 1 into *bad_flag (integer atomicOr; bad_flag may
 *   be NULL: then only the zero is written).  The caller zeroes *bad_flag beforehand and reads it when it chooses.
 * E == 0 succeeds and launches nothing. */
int tfgx_edge_dot_f32(const int32_t* row, const int32_t* col, int64_t E,
                      const float* a, int64_t lda, int64_t n_a,
                      const float* b, int64_t ldb, int64_t n_b,
                      int64_t F, float* out /* [E] */,
                      int32_t* bad_flag /* device int32 or NULL */,
                      tfgx_stream_t stream);

/* host: the candidate pair every kernel below tests for (seed, slot, attempt).  With h(key, i) the library's mixer:
 *   key = h(seed, low 32 bits of slot) << 32 | h(seed ^ 0x9E3779B97F4A7C15, high 32 bits of slot ^ the first word)
 *   u = (uint64(h(key, 2 attempt)) * num_nodes) >> 32,   v = (uint64(h(key, 2 attempt + 1)) * num_nodes) >> 32.
 * Bias: a node receives floor or ceil of 2^32 / num_nodes of the 2^32 words, so node probabilities differ from
 * 1 / num_nodes by at most num_nodes / 2^32 RELATIVE (5e-4 at 2.4 M nodes, below 0.5 at the 2^31 limit).
 * num_nodes must be in [1, 2^31) and attempt in [0, 2^31); otherwise *u = *v = -1. */
void tfgx_negative_draw(uint64_t seed, uint64_t slot, uint32_t attempt, int64_t num_nodes, int32_t* u, int32_t* v);

/* Slot s in [0, num_samples) writes (out_row[s], out_col[s]) = the first accepted draw of slot slot_base + s.
 *   adj_ptr == adj_col == NULL (no filter): attempt 0 is returned as drawn, self-pairs included, undirected ignored.
 *   undirected == 1: the pair is ordered (min, max); u == v and pairs present in the (upper-triangular) adjacency are rejected.
 *   undirected == 0: (u, v) as drawn; u == v and pairs present in the (directed) adjacency are rejected.
 *   A slot that exhausts max_attempts (>= 1) writes (-1, -1) and adds 1 to *n_failed (integer atomicAdd; the caller
 *   zeroes the word beforehand). */
int tfgx_negative_sample_pairs(int64_t num_samples, int64_t num_nodes,
                               const int32_t* adj_ptr, const int32_t* adj_col, /* both NULL: no filter */
                               int32_t undirected, uint64_t seed, uint64_t slot_base, int32_t max_attempts,
                               int32_t* out_row, int32_t* out_col,
                               int32_t* n_failed /* device int32 */, tfgx_stream_t stream);

/* Slot s writes out_col[s] = v of the first draw of slot slot_base + s with v != start[s] and (start[s], v) absent from
 * the (directed) adjacency.  adj_ptr == adj_col == NULL: v of attempt 0, unfiltered (it may equal start[s]).
 *   A slot that exhausts max_attempts writes -1 and adds 1 to *n_failed.  A start node outside [0, num_nodes) writes -1
 *   and ORs TFGX_NEGATIVE_BAD_START into *n_failed: the caller that reads the word reports TFGX_ERR_INDEX. */
int tfgx_negative_sample_from(const int32_t* start, int64_t num_samples, int64_t num_nodes,
                              const int32_t* adj_ptr, const int32_t* adj_col,
                              uint64_t seed, uint64_t slot_base, int32_t max_attempts,
                              int32_t* out_col, int32_t* n_failed, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_LINKPRED_H */
