/*
 * tfgx_nbrstatic — fixed-shape minibatch neighbour sampling: every size of a sample is a capacity the host knows from
 * (number of seeds, fan-outs) alone, every run-time size lives in device memory, and nothing is read back.  A whole
 * sample -> forward -> backward -> optimizer step is then a fixed launch sequence that a hipGraph can replay.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header and its TFGX_ABI_VERSION do not change.
 *
 * Reference: tf_geometric/utils/graph_utils.py:630-772 (RandomNeighborSampler) and demo/demo_graph_sage.py
 * (num_sampled_neighbors_list = [25, 10]: one sampled block per layer).
 *
 * The layout.  A hop over R rows with fan-out k has an edge capacity E = R * k, E slots for new nodes and S sink rows
 * (S = R, or 0 when k == 0): R' = R + E + S virtual nodes, in the order [rows | new-node slots | sinks].  `node` int32 [R']
 * holds the global id of a live virtual node and -1 for a dead one (a dead seed slot, an unused new-node slot, a sink).
 * The hop's block is a SQUARE graph on R' nodes with exactly E edges in CSR order by destination:
 *   [0, total)   the sampled edges: destination = the row's position, source = the neighbour's virtual id (new nodes take
 *                R, R + 1, ... in order of their first occurrence, the rule of tfgx_nbrblock_relabel);
 *   [total, E)   unit-weight self-loops on the sink rows R + E, R + E + 1, ..., filled in order with at most k per sink.
 * No row of a block is longer than k.  A live row draws what tfgx_nbrblock_sample_rows gives that node with the same seed,
 * count rule and replace_when_short, bit for bit (both run the per-row bodies of csrc/tfgx_sample_rows.h); a dead row
 * draws nothing.
 *
 * The seed is ONE uint64 in device memory that the kernels read when they run; hop h (0 = next to the seeds) samples with
 * (seed + (h + 1) * 0x9E3779B97F4A7C15) mod 2^63, the mixing of utils.hop_seed, done on the device.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.
 * Zero-size calls succeed and launch nothing.  Integer atomics only (min / or, both commutative): nothing depends on the
 * order they land in and every output is bit-identical from run to run.  Every launch is on the one given stream, in a
 * fixed order.  The relabel table is the persistent table of tfgx_nbrblock.h (entries TFGX_NBRBLOCK_EMPTY between calls;
 * tfgx_nbrblock_reset over `node` empties what a call wrote and skips -1).
 */
#ifndef TFGX_NBRSTATIC_H
#define TFGX_NBRSTATIC_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_NBRSTATIC_ABI_VERSION 1
int tfgx_nbrstatic_version(void);   /* the TFGX_NBRSTATIC_ABI_VERSION the library was built with */

/* A dead entry of a seed list / of `node`. */
#define TFGX_NBRSTATIC_DEAD (-1)

/* Bits of the device word `flag` (OR-ed in; the caller zeroes the word): the values of TFGX_NBRBLOCK_BAD_*. */
#define TFGX_NBRSTATIC_BAD_RANGE 1     /* a seed that is neither TFGX_NBRSTATIC_DEAD nor in [0, n_nodes) */
#define TFGX_NBRSTATIC_BAD_REPEAT 2    /* a seed that occurs earlier in the list */

/* Enter the seeds: node[j] = seeds[j] and table[seeds[j]] = j for a live seed, node[j] = -1 for a dead slot (anywhere in the
 * list).  A seed outside [0, n_nodes) other than -1 raises TFGX_NBRSTATIC_BAD_RANGE, a seed that occurs earlier in the list
 * TFGX_NBRSTATIC_BAD_REPEAT; either slot becomes dead (the FIRST occurrence of a repeated seed stays live: an integer
 * atomicMin of the position decides, whatever order the lanes arrive in).  The table must be all TFGX_NBRBLOCK_EMPTY.
 * Two launches. */
int tfgx_nbrstatic_seeds(int32_t* table, int64_t n_nodes, const int32_t* seeds, int64_t B, int32_t* node, int32_t* flag,
                         tfgx_stream_t stream);

/* Bytes of scratch tfgx_nbrstatic_hop needs for R rows at fan-out k. */
size_t tfgx_nbrstatic_hop_workspace_bytes(int64_t R, int32_t k);

/* One hop.  R rows node[0 .. R) (live or -1), fan-out k: E = R * k, S = (k > 0 ? R : 0), R' = R + E + S.
 *   row_ptr [n_nodes + 1], col / w [row_ptr[n_nodes]]: the graph's CSR by destination (w NULL: all ones).
 *   table [n_nodes]: the relabel table; holds the virtual id of every live node[0 .. R) on entry and of every live
 *                node[0 .. R') on return.
 *   node [R']: entries [R, R') are written — the new nodes in first-occurrence order, then -1.
 *   replace_when_short: a live row with d > 0 neighbours draws k of them with replacement when d < k (else min(d, k)).
 *   seed: one uint64 on the device, read by the kernels; hop: the hop's index (0 = next to the seeds) for the mixing above.
 *   block_row_ptr [R' + 1], block_row [E], block_col [E], block_w [E]: the block (layout above).
 *   counts [2]: (sampled edges `total`, new nodes), on the device.
 * E == 0 (R == 0 or k == 0) writes block_row_ptr and counts only.  R' must fit int32. */
int tfgx_nbrstatic_hop(const int32_t* row_ptr, const int32_t* col, const float* w /* or NULL */, int64_t n_nodes,
                       int32_t* table, int32_t* node, int64_t R, int32_t k, int32_t replace_when_short,
                       const uint64_t* seed, int32_t hop, int32_t* block_row_ptr, int32_t* block_row, int32_t* block_col,
                       float* block_w, int32_t* counts, void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

/* Bytes of scratch tfgx_nbrstatic_transpose needs for E edges over n nodes. */
size_t tfgx_nbrstatic_transpose_workspace_bytes(int64_t E, int64_t n);

/* The by-source plan of a block without a host read: a stable sort of the E edge positions by block_col.
 *   t_row_ptr [n + 1]: t_row_ptr[v] = first sorted position whose source is >= v;
 *   t_col [E]: the destination (block_row) of the edge at each sorted position;  t_perm [E]: its position in the block.
 * What tfgx_build_csr_by_dst writes for the flipped list, bit for bit, minus its id validation (and its host read): the ids
 * are the sampler's own, every one in [0, n). */
int tfgx_nbrstatic_transpose(const int32_t* block_row, const int32_t* block_col, int64_t E, int64_t n, int32_t* t_row_ptr,
                             int32_t* t_col, int32_t* t_perm, void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

/* out[i, :F] = x[idx[i], :F] for idx[i] >= 0 and zeros for idx[i] < 0, i in [0, M).  x [rows ldx floats apart], out [M rows
 * ldo floats apart].  A lane takes a 16-byte chunk of columns where x and out allow it (ldx % 4 == 0, ldo % 4 == 0, both
 * bases on 16 bytes; the F % 4 last columns take a scalar pass), else one column.  A dead row loads row 0 and drops the value
 * with a select: no load is predicated.  An id >= the table's rows is the caller's error (not checked). */
int tfgx_nbrstatic_gather_rows_f32(const float* x, int64_t ldx, const int32_t* idx, int64_t M, int64_t F, float* out,
                                   int64_t ldo, tfgx_stream_t stream);

/* The fused input hop over `node` (tfgx_samplereduce_f32 with the seed read from the device): out[i, :F] = reduce_j
 * w_j * x[c_j, :F] over the neighbours node[i] draws at fan-out k with hop seed `hop` of *seed.  A dead row (node[i] < 0)
 * gives a row of zeros and count 0 and raises no flag; an id >= n_nodes writes nothing and raises TFGX_NBRSTATIC_BAD_RANGE.
 * Every other argument, limit (0 <= k <= TFGX_SAMPLEREDUCE_MAX_DRAWS) and bit as tfgx_samplereduce_f32. */
int tfgx_nbrstatic_input_hop_f32(const int32_t* row_ptr, const int32_t* col, const float* w /* or NULL */, int64_t n_nodes,
                                 const int32_t* node, int64_t n_rows, int32_t k, int32_t replace_when_short,
                                 const uint64_t* seed, int32_t hop, const float* x, int64_t ldx, int64_t F,
                                 int32_t op /* TFGX_SUM | TFGX_MEAN */, float* out, int64_t ldo,
                                 int32_t* out_count /* [n_rows] or NULL */, int32_t* bad_flag, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_NBRSTATIC_H */
