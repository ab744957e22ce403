/*
 * tfgx_asapstatic — the three device pieces of one fixed-shape ASAP level (nn.asap_static): a static batch
 * (include/tfgx_collate_static.h) in, a static batch out, at sizes the host knows.  Nothing is read back and nothing is sorted,
 * so a hierarchical classifier with ASAP pooling over fixed-shape batches is a fixed launch sequence that a hipGraph can replay.
 * Exported from libtfgx.so next to the entry points of tfgx.h; that header, tfgx_asap.h, tfgx_pool_static.h and
 * tfgx_dense_pool_static.h and their versions do not change.
 *
 * Reference: tf_geometric/nn/pool/asap.py:19-131 (the level), nn/pool/cluster_pool.py:32-46 (S^T A S and its edge list).
 *
 * A static batch keeps its self-loops (padded unit loops on the sinks; one live unit loop per cluster after an ASAP level), and
 * ASAP works on the list WITHOUT self-loops.  The list is never compacted here: an edge with row == col is ABSENT — (a) skips it,
 * (b) skips it, the caller gives it weight 0 elsewhere.
 *
 * The parent batch has B slots and N = n_cap rows with a CSR plan by destination (row_ptr [N + 1], col [E], E = e_cap).  The
 * selection (tfgx_static_pool_table / tfgx_static_pool_select of tfgx_pool_static.h, called with THIS level's capacities) gives
 * pooled_row_ptr [B + 2], node_index [n_cap'] (pooled row -> parent row, -1 dead) and the pooled node_graph_index [n_cap'].
 * Slot g keeps m_g = pooled_row_ptr[g + 1] - pooled_row_ptr[g] clusters, at most K = K_blk (host arithmetic) of them.
 *
 * Conventions: those of tfgx.h (device pointers owned by the caller, asynchronous on `stream`, 0 = ok or a TFGX_ERR_* code with
 * text in tfgx_last_error()).  Every refusal happens on the host before any device work and names its argument.  Zero-size
 * calls succeed.  No float atomics and no global atomics: every output is a pure function of the inputs (the optional bad_flag
 * of (a) is ORed with an integer atomic exactly as tfgx_asap_attend_f32 does it; nn.asap_static passes NULL).  Every index read
 * from device memory is held to its array's bounds before it is used as an address, and every store to the capacities; a load
 * that may be out of range is clamped, not predicated.
 */
#ifndef TFGX_ASAP_STATIC_H
#define TFGX_ASAP_STATIC_H

#include "tfgx_collate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header: bumped whenever one of its signatures changes. */
#define TFGX_ASAPSTATIC_ABI_VERSION 1
int tfgx_asapstatic_version(void);   /* the TFGX_ASAPSTATIC_ABI_VERSION the library was built with */

/* The most clusters per graph: TFGX_SEGGRAM_MAX_K of tfgx_seggram.h (a row of a block is one wave ballot). */
#define TFGX_ASAPSTATIC_MAX_K 64

/* The most feature columns of (a): TFGX_ASAP_MAX_FEATURES of tfgx_asap.h (the same kernel). */
#define TFGX_ASAPSTATIC_MAX_FEATURES 256

/* The most slots the one-workgroup scan of (c) covers. */
#define TFGX_ASAPSTATIC_MAX_SLOTS 1048576

/* (a) The 1-hop attention forward, ONE launch: the contract of tfgx_asap_attend_f32 (tfgx_asap.h; the same kernel body) plus
 *   skip_self_loops != 0 : an edge with col_e == i (its own row) contributes nothing — not to the maximum, not to the
 *                          denominator, not to c — and p = p_drop = 0 is written for it.  It is not a bad edge.
 *   seed_dev             : NULL: the by-value `seed`.  Otherwise ONE uint64 in device memory that the kernel reads (hipGraph
 *                          replays: the captured sequence leaves a fresh value there before every replayed launch); `seed` is
 *                          ignored.
 * The dropout position of an edge is its CSR position, E + i for the implicit self edge of row i — absent edges keep theirs.
 * With skip_self_loops == 0 and seed_dev == NULL the outputs are those of tfgx_asap_attend_f32 bit for bit; so they are with
 * skip_self_loops != 0 on a list without self-loops.  tfgx_asap_attend_backward_f32 is a valid backward as it is (a skipped edge
 * has p = 0); nn.asap_static uses (a') below, which is exact where that one rounds to 0.  N == 0: nothing is done.  F == 0: only the weights are written. */
int tfgx_asapstatic_attend_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E,
                               const float* x, int64_t ldx, int64_t F,
                               const float* sq, const float* sh, const float* bias /* device, one float */,
                               float drop_rate, uint64_t seed, const uint64_t* seed_dev /* device or NULL */,
                               int32_t skip_self_loops,
                               float* c, int64_t ldc, float* p, float* p_self,
                               float* p_drop /* or NULL */, float* p_self_drop /* or NULL */,
                               int32_t* bad_flag /* device int32 or NULL */, tfgx_stream_t stream);

/* (a') The backward of the weights of (a): the contract of tfgx_asap_attend_backward_f32 (tfgx_asap.h) — dp, dp_self in, ds, ds_self,
 * dsq out, p_drop / p_self_drop NULL when no dropout was applied (p_self_drop decides; with E == 0 it may come alone) — plus skip_self_loops, in a form that never subtracts the row's
 * weights from 1.  With u_e = k_e dp_e and r = u of the self edge
 *   ds_e = p_e ((u_e - r) - sum_j p_j (u_j - r) + r * 1e-8 / D) * (z_e > 0 ? 1 : 0.2)
 * which equals p_e (u_e - sum_j p_j u_j) since sum_j p_j = 1 - 1e-8 / D; m and D are recomputed from sq, sh, bias.  A row of ONE
 * term (a graph pooled to one node: p_self = 1 / (1 + 1e-8) = 1.0f in float32) thus keeps the gradient the epsilon leaves it,
 * which tfgx_asap_attend_backward_f32 rounds to 0.  An edge with p = 0 (absent, invalid or underflowed) gets ds = 0.
 * ONE launch.  N == 0: nothing is done. */
int tfgx_asapstatic_attend_backward_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E,
                                        const float* sq, const float* sh, const float* bias,
                                        const float* p, const float* p_self,
                                        const float* p_drop /* or NULL */, const float* p_self_drop /* or NULL */,
                                        const float* dp, const float* dp_self, int32_t skip_self_loops,
                                        float* ds, float* ds_self, float* dsq, tfgx_stream_t stream);

/* (b) The dense assignment S [N, K] on leading dimension lds, TWO launches (zero S, scatter).  S is zero everywhere except, for
 * pooled row r = pooled_row_ptr[g] + c of slot g = pooled_node_graph_index[r] with centre i = node_index[r]:
 *   S[col_e, c] = the sum of p[e] over the edges e of row i with that column, in CSR order (duplicates add up in that order),
 *                 without the edges with col_e == i when skip_self_loops != 0;
 *   S[i, c]    += p_self[i], last.
 * p / p_self are what multiplied the features: the p_drop / p_self_drop of (a) under dropout.  A wave owns a pooled row; the
 * lane holding the FIRST edge of a column sums that column over the whole row and stores it once, so nothing is read back,
 * nothing is accumulated in memory and no two lanes store one element (distinct centres own distinct columns c).  The work of a
 * row of L edges grows as L * L / 64: the rows of a static batch are as short as the store's largest degree.
 * A pooled row that is dead (node_index < 0), whose slot is outside [0, B), whose c is outside [0, K) or whose centre is outside
 * [0, N) writes nothing; a CSR span outside [0, E] is an empty row, a column outside [0, N) is skipped.
 * Refused, before S is touched: a negative size or one not fitting int32, K > TFGX_ASAPSTATIC_MAX_K, lds < K, a null pointer that
 * the sizes need (S whenever N, K > 0; the others whenever m_rows > 0, col and p only with E > 0).
 * N == 0 or K == 0: nothing is done.  m_rows == 0: S is zeroed. */
int tfgx_asapstatic_assign_f32(const int32_t* row_ptr, const int32_t* col, int64_t N, int64_t E,
                               const float* p, const float* p_self, int32_t skip_self_loops,
                               const int32_t* node_index /* [m_rows] */, const int32_t* pooled_node_graph_index /* [m_rows] */,
                               const int32_t* pooled_row_ptr /* [B + 2] */, int64_t B, int64_t m_rows, int64_t K,
                               float* S, int64_t lds, tfgx_stream_t stream);

/* (c) Pooled edges and both plans from the blocks P [B K, K] (rows [g K, (g + 1) K) are slot g's S_g^T (A1 S)_g, what
 * tfgx_segment_gram_f32 writes with G = B) and pooled_row_ptr: the ragged sibling of tfgx_dense_pool_static — slot g owns m_g
 * rows, not K.  With m_live = pooled_row_ptr[B] the layout is
 *   edges [0, e_live)      : slot by slot; for pooled row r = pooled_row_ptr[g] + c1 (c1 < m_g) first the entries c2 != c1,
 *                            c2 < m_g, with P[g K + c1, c2] != 0.0f (C's comparison: -0.0 is no edge, a NaN is one) in column
 *                            order — row = r, col = pooled_row_ptr[g] + c2, edge_src = (g K + c1) K + c2 (the flat position in a
 *                            P of ldp == K) —, then the row's unit self-loop — row = col = r, edge_src = -1 —, whatever
 *                            P[g K + c1, c1] holds.  edge_graph_index = g.  This is the order in which the CSR plan of nn.asap's
 *                            pooled list walks a row;
 *   edges [e_live, e_cap)  : edge q is a unit self-loop on sink t = (q - e_live) / d: row = col = n_cap_out - sinks + t,
 *                            edge_src = -1, edge_graph_index = B (the rule of tfgx_collate_static.h);
 *   the two plans          : what tfgx_build_csr_by_dst gives for the emitted [2, e_cap] list and for its flip.  The list is
 *                            sorted by row, so the plan by row has the identity permutation; in the plan by column a stable sort
 *                            puts the self-loop of column c2 between the rows below and above c2, so it ranks every entry of a
 *                            slot in column-major order of the block with its diagonal set; dead non-sink rows are empty, sink
 *                            rows have a closed form, the padded tail is the identity — no sort;
 *   counts [4]             : counts[2] = e_live is written; the other three are the selection's (live graphs, m_live, flags).
 * No weights are written: the pooled weight of edge q is P at edge_src[q], 1.0f where edge_src[q] < 0.
 * Launches: a FIXED sequence of three with no host read between them (count: a workgroup per slot, a row's mask is one wave
 * ballot; scan: one workgroup over the B slots; emit: a workgroup per slot, then workgroups for the dead and sink rows' row_ptr
 * and for the padded tail).  K == 0: two launches (every slot is empty). */
typedef struct tfgx_asapstatic_edges_args {
    const float* P;                  /* [B K, K] rows on leading dimension ldp (floats); not read when K == 0 */
    int64_t ldp;
    const int32_t* pooled_row_ptr;   /* [B + 2] */
    int64_t B;
    int64_t K;                       /* K_blk: the most rows of a slot */
    /* the pooled capacities */
    int64_t n_cap_out;               /* pooled rows, the sinks included */
    int64_t e_cap;                   /* pooled edges: at least K * (n_cap_out - sinks) */
    int64_t sinks;                   /* P' */
    int64_t sink_degree;             /* d */
    /* the outputs */
    int32_t* out_row;                /* [e_cap] */
    int32_t* out_col;                /* [e_cap] */
    int32_t* out_edge_src;           /* [e_cap] */
    int32_t* out_edge_graph_index;   /* [e_cap] */
    const tfgx_collate_plan* plan;   /* by row: out_row_ptr [n_cap_out + 1], out_col / out_perm [e_cap]; the ds_* members are not read */
    const tfgx_collate_plan* plan_t; /* by column */
    int32_t* counts;                 /* [4]: counts[2] is written */
    void* workspace;
    size_t workspace_bytes;          /* at least tfgx_asapstatic_edges_workspace_bytes(B) */
} tfgx_asapstatic_edges_args;

size_t tfgx_asapstatic_edges_workspace_bytes(int64_t B);

/* Refused on the host, with the member named: a null member that the sizes need (pooled_row_ptr, counts, both plans with their
 * out_row_ptr and the workspace always), a negative size, a size not fitting int32 (B K K among them),
 * B > TFGX_ASAPSTATIC_MAX_SLOTS, K > TFGX_ASAPSTATIC_MAX_K, ldp < K, sink_degree < 1, sinks > n_cap_out,
 * sinks * sink_degree < e_cap, e_cap < K * (n_cap_out - sinks) (sum m_g^2 <= K sum m_g: such capacities cannot overflow), a
 * workspace that is too small.  B == 0 with n_cap_out == 0 and e_cap == 0 and no output given launches nothing. */
int tfgx_asapstatic_edges(const tfgx_asapstatic_edges_args* args, tfgx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TFGX_ASAP_STATIC_H */
