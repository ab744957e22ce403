/*
 * tfgx_asap — the two hot paths of ASAP pooling: the fused 1-hop attention (scores, per-row softmax, dropout and the
 * weighted feature sum in one launch, with the one launch its backward needs), and a sparse S^T A S by expand - sort -
 * compress (the coarsened adjacency of cluster_pool).  Exported from libtfgx.so next to the entry points of tfgx.h; that
 * header and its version do not change.
 *
 * Reference: tf_geometric/nn/pool/asap.py:67-85 (two [E', A] gathers, a concat, a [2A, 1] product, leaky_relu, a three-op
 * segment_softmax, dropout, a gather - multiply - segment sum) and nn/pool/cluster_pool.py:32-38 (a dense [N, N] adjacency,
 * two sparse - dense products, a scan of the dense [K, K] result).
 *
 * No float atomics, no data-dependent reduction order: results are bit-identical from run to run.  Nothing is allocated.
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code
 * with text in tfgx_last_error(), host-side argument checks before any device work, zero sizes succeed without a launch).
 */
#ifndef TFGX_ASAP_H
#define TFGX_ASAP_H

#include "tfgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_ASAP_ABI_VERSION 1
int tfgx_asap_version(void);   /* the TFGX_ASAP_ABI_VERSION the library was built with */

/* ---- (a) the 1-hop attention ----------------------------------------------------------------------------------------------
 * A CSR plan by destination row over N nodes (row_ptr [N + 1], col [E]; the self edge of every row is IMPLICIT and comes
 * first in the order of summation).  sq [N], sh [N]: the two per-node halves of the score, bias: ONE float in device memory.
 *   z_e = sq[i] + sh[col_e] + bias      s_e = z_e > 0 ? z_e : 0.2 z_e             (e = the self edge: col_e = i)
 *   m_i = max_e s_e      p_e = exp(s_e - m_i) / (sum_e exp(s_e - m_i) + 1e-8)
 *   k_e = tfgx_dropout_keep(seed, position, drop_rate) / (1 - drop_rate)           (1 when drop_rate == 0)
 *         position = the CSR position of the edge, E + i for the self edge of row i
 *   c_i = sum_e k_e p_e x[col_e]
 * One wave owns a row and walks it 64 edges at a time with the running (m, sum, c) carried, so a row of any length works;
 * the sum is kept WITHOUT the running maximum's own 1 and a chunk is summed before it is folded in.
 * x is read once; nothing of size [E, F] is made.  F is in [0, TFGX_ASAP_MAX_FEATURES].
 */
#define TFGX_ASAP_MAX_FEATURES 256

/* Forward.  c [N, F] (ldc >= F), p [E] (CSR order) and p_self [N] are written for every row and edge: p is the softmax
 * BEFORE dropout.  p_drop [E] and p_self_drop [N] receive k_e p_e; they are required when drop_rate > 0 and may be NULL
 * otherwise (they would equal p and p_self).  drop_rate in [0, 1).
 *   A row_ptr span that is not inside [0, E] or runs backwards is treated as an empty row, a column outside [0, N) as an edge
 *   of weight 0; either ORs 1 into *bad_flag (never an out-of-range access).  bad_flag may be NULL; the caller zeroes it.
 *   N == 0: nothing is done.  F == 0: only the weights are written. */
int tfgx_asap_attend_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E,
                         const float* x, int64_t ldx, int64_t F,
                         const float* sq, const float* sh, const float* bias /* device, one float */,
                         float drop_rate, uint64_t seed,
                         float* c, int64_t ldc, float* p, float* p_self,
                         float* p_drop /* or NULL */, float* p_self_drop /* or NULL */,
                         int32_t* bad_flag /* device int32 or NULL */, tfgx_stream_t stream);

/* Backward of the weights.  dp [E], dp_self [N]: the gradient of the loss with respect to k_e p_e, that is
 * <d c_i, x[col_e]> (tfgx_sddmm_f32 / a row-wise dot).  With t_i = sum_e (k_e p_e) dp_e over the row, self edge included:
 *   ds_e = ((k_e p_e) dp_e - p_e t_i) * (z_e > 0 ? 1 : 0.2)         ds [E], ds_self [N]
 *   dsq_i = sum_e ds_e                                               dsq [N]
 * (exact with the epsilon in the denominator; the maximum is a stop-gradient).  d sh is the column-wise (transposed) sum
 * of ds plus ds_self, d bias the sum of dsq: both left to the caller's existing reductions.
 * p_drop / p_self_drop == NULL: no dropout was applied (k_e = 1).  Invalid spans and columns are skipped as in the forward.
 * N == 0: nothing is done. */
int tfgx_asap_attend_backward_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E,
                                  const float* sq, const float* sh, const float* bias,
                                  const float* p, const float* p_self,
                                  const float* p_drop /* or NULL */, const float* p_self_drop /* or NULL */,
                                  const float* dp, const float* dp_self,
                                  float* ds, float* ds_self, float* dsq, tfgx_stream_t stream);

/* ---- (b) P = S^T A S, sparse -----------------------------------------------------------------------------------------------
 * S [N, K] in CSR by node: s_row_ptr [N + 1], s_col [nnz_S] (cluster ids), s_val [nnz_S] (NULL: ones).  An entry whose
 * cluster id is outside [0, K) is not part of S (a caller may mark unassigned entries with -1 instead of compacting).
 * A [N, N] as an edge list: a_row [E], a_col [E], a_val [E] (NULL: ones); duplicates are separate terms.
 * The STRUCTURE of S is trusted (build it with tfgx_build_csr_by_dst, which validates): s_row_ptr must be non-decreasing with
 * s_row_ptr[0] >= 0 and s_row_ptr[N] <= the length of s_col / s_val (the header takes no nnz_S, so the spans cannot be checked
 * here); only the VALUES of s_col and the endpoints of A are validated.
 *
 *   count   s_deg[u] = the valid entries of S's row u; offsets = the exclusive scan of s_deg[a_row[e]] * s_deg[a_col[e]];
 *           *total (HOST memory) = offsets[E].  Synchronises the stream once.  An edge endpoint outside [0, N) ->
 *           TFGX_ERR_INDEX; a total above 2^31 - 1 -> TFGX_ERR_INVALID_ARG.
 *   emit    edge e writes, for its i-th entry (u, c1) and j-th entry (v, c2), the key c1 << 32 | c2 and the value
 *           (S[u, c1] * a_e) * S[v, c2] at position offsets[e] + i * s_deg[v] + j of the workspace: the order of emission is a
 *           function of the inputs alone.
 *   reduce  one stable radix sort of the keys, then one sequential float32 chain per run of equal keys in sorted order.  A
 *           sum equal to 0.0 is dropped, and with drop_diagonal != 0 so is every c1 == c2.  Writes the (row, col)-sorted
 *           list out_row / out_col / out_val (capacity: total entries each), out_row_ptr [K + 1] and *out_count (DEVICE
 *           int32): the caller reads the count, its second and last synchronisation.
 * emit and reduce share one workspace of tfgx_spasp_workspace_bytes(total, K) bytes (0 for total == 0, and for a total or K
 * that is refused); count needs tfgx_spasp_count_workspace_bytes(N, E).  N, K, E and nnz_S fit int32.
 */
size_t tfgx_spasp_count_workspace_bytes(int64_t N, int64_t E);
size_t tfgx_spasp_workspace_bytes(int64_t total, int64_t K);

int tfgx_spasp_count(const int32_t* s_row_ptr, const int32_t* s_col, int64_t N, int64_t K,
                     const int32_t* a_row, const int32_t* a_col, int64_t E,
                     int32_t* s_deg /* [N] */, int64_t* offsets /* [E + 1] */, int64_t* total /* host */,
                     void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

int tfgx_spasp_emit(const int32_t* s_row_ptr, const int32_t* s_col, const float* s_val /* or NULL */, int64_t N, int64_t K,
                    const int32_t* a_row, const int32_t* a_col, const float* a_val /* or NULL */, int64_t E,
                    const int32_t* s_deg, const int64_t* offsets, int64_t total,
                    void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

int tfgx_spasp_reduce(int64_t total, int64_t K, int32_t drop_diagonal,
                      int32_t* out_row, int32_t* out_col, float* out_val, int32_t* out_row_ptr /* [K + 1] */,
                      int32_t* out_count /* device int32 */, void* workspace, size_t workspace_bytes, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_ASAP_H */
