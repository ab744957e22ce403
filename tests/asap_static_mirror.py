# coding=utf-8
"""A numpy mirror of include/tfgx_asap_static.h: the dense assignment S (piece b, float32 in the header's order of summation)
and the pooled edge list with both plans (piece c), from the blocks P [B K, K], the selection's pooled_row_ptr and counts and
the pooled capacities; and the host arithmetic of StaticBatchGraph.asap_pooled_capacities.  It follows the header's words, not
the kernels' code: the edges are written row by row, and the two plans are built from the header's description of them (per-slot
column-major order, closed-form tails) — tests/test_asap_static_abi.py holds them to a stable sort (test_drop_edge_abi.mirror_plan)."""
import math

import numpy as np


def mirror_clusters(n, k=None, ratio=None):
    """m_g of a graph of n nodes: the rule of tfgx_segment_topk (asap_mirror.topk_select's)."""
    if k is not None:
        return min(int(k), int(n))
    return min(int(n), int(np.ceil(np.float32(n) * np.float32(ratio))))


def mirror_asap_capacities(B, parent_max_nodes, n_max, sink_degree, k=None, ratio=None):
    """(K_blk, max_nodes, max_edges, sinks, n_cap, e_cap) of StaticBatchGraph.asap_pooled_capacities for a parent batch of B
    slots and parent_max_nodes live rows at most whose largest graph has n_max nodes."""
    import fractions
    K = mirror_clusters(n_max, k, ratio)
    if k is not None:
        m_max = min(parent_max_nodes, B * int(k))
    else:
        bound = fractions.Fraction(float(np.float32(ratio))) * parent_max_nodes * (1 + fractions.Fraction(1, 1 << 22))
        m_max = min(parent_max_nodes, math.ceil(bound) + B)
    max_edges = K * m_max
    sinks = max(1, -(-max_edges // sink_degree))
    return K, m_max, max_edges, sinks, m_max + sinks, max_edges


def mirror_assignment(row_ptr, col, p, p_self, node_index, pooled_ngi, pooled_row_ptr, B, K, skip_self_loops=True):
    """S [N, K] float32: for pooled row r of slot g with centre i, column c = r - pooled_row_ptr[g] receives the weights of
    row i's edges per column in CSR order (float32 running sums), and p_self[i] last on S[i, c]."""
    N = len(row_ptr) - 1
    S = np.zeros((N, K), np.float32)
    for r, i in enumerate(node_index):
        g = pooled_ngi[r]
        if i < 0 or g < 0 or g >= B:
            continue
        c = r - pooled_row_ptr[g]
        assert 0 <= c < K
        for e in range(row_ptr[i], row_ptr[i + 1]):
            if skip_self_loops and col[e] == i:
                continue
            S[col[e], c] = np.float32(S[col[e], c] + p[e])
        S[i, c] = np.float32(S[i, c] + p_self[i])
    return S


def mirror_asap_layout(P, pooled_row_ptr, counts, K, n_cap_out, e_cap, sinks, sink_degree):
    P = None if K == 0 else np.asarray(P, np.float32).reshape(-1, K)
    prp = np.asarray(pooled_row_ptr, np.int64)
    B = prp.shape[0] - 2
    m_rows = n_cap_out - sinks
    m_live = int(prp[B]) if K else 0
    assert sinks * sink_degree >= e_cap and e_cap >= K * m_rows and m_live <= m_rows
    rows, cols, src, egi = [], [], [], []
    for g in range(B):
        p0, m_g = int(prp[g]), int(prp[g + 1] - prp[g]) if K else 0
        assert 0 <= m_g <= K
        for c1 in range(m_g):
            for c2 in range(m_g):
                if c2 != c1 and P[g * K + c1, c2] != np.float32(0.0):      # -0.0 is no edge, a NaN is one
                    rows.append(p0 + c1), cols.append(p0 + c2), src.append((g * K + c1) * K + c2), egi.append(g)
            rows.append(p0 + c1), cols.append(p0 + c1), src.append(-1), egi.append(g)      # the unit self-loop, last in its row
    rows, cols, src, egi = (np.asarray(a, np.int64) for a in (rows, cols, src, egi))
    e_live = rows.shape[0]
    assert e_live <= e_cap
    q = np.arange(e_live, e_cap)
    sink = m_rows + (q - e_live) // sink_degree
    edge_index = np.stack([np.concatenate([rows, sink]), np.concatenate([cols, sink])]).astype(np.int32)
    # the two plans as the header words them: rows [m_live, m_rows] start at e_live, sink t at e_live + min(e_cap - e_live, t d);
    # the plan by row is the list itself; the plan by column holds a slot's entries inside the slot's own edge range in
    # column-major order OF THE BLOCK (the self-loop of c2 between the rows below and above c2) — a lexsort of (column, row)
    # inside each slot here, where the kernel uses popcounts; the padded tail is the identity
    t = np.arange(sinks + 1, dtype=np.int64)
    tail_ptr = e_live + np.minimum(e_cap - e_live, t * sink_degree)
    plans = []
    for by_col in (False, True):
        key, other = (cols, rows) if by_col else (rows, cols)
        row_ptr = np.full(n_cap_out + 1, e_live, np.int64)
        row_ptr[:m_live + 1] = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=m_live)[:m_live])])
        row_ptr[m_rows:] = tail_ptr
        perm = np.arange(e_cap, dtype=np.int64)
        if by_col:
            at = 0
            for g in range(B):
                n = int((egi == g).sum())                        # the slot's edges are [at, at + n) of the list
                c1, c2 = rows[at:at + n] - prp[g], cols[at:at + n] - prp[g]
                perm[at:at + n] = at + np.lexsort((c1, c2))      # by column, then by row
                at += n
        col = np.concatenate([other, sink])[perm]
        plans.append((row_ptr.astype(np.int32), col.astype(np.int32), perm.astype(np.int32)))
    pc = np.asarray(counts, np.int32)
    return dict(plan=plans[0], plan_t=plans[1], edge_index=edge_index,
                edge_src=np.concatenate([src, np.full(q.shape[0], -1)]).astype(np.int32),
                edge_graph_index=np.concatenate([egi, np.full(q.shape[0], B)]).astype(np.int32),
                counts=np.asarray([pc[0], pc[1], e_live, pc[3]], np.int32), e_live=e_live, m_live=m_live)
