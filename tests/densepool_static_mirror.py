# coding=utf-8
"""A numpy mirror of include/tfgx_dense_pool_static.h: the pooled static batch of one fixed-shape DiffPool / MinCutPool level,
from the diagonal blocks P [B K, K] of S^T A S, the parent's graph_mask and counts and the pooled capacities.  It follows the
header's words, not the kernels' code: the edges are np.nonzero of the live blocks in slot order, and the two plans come from the
header's closed forms — tests/test_dense_pool_static_abi.py holds them to a stable sort (test_drop_edge_abi.mirror_plan)."""
import numpy as np


def mirror_dense_capacities(B, K, sink_degree, drop_diagonal=False):
    """(max_nodes, max_edges, sinks, n_cap, e_cap) of StaticBatchGraph.dense_pooled_capacities."""
    max_nodes, max_edges = B * K, B * K * (K - 1 if drop_diagonal else K)
    sinks = max(1, -(-max_edges // sink_degree))
    return max_nodes, max_edges, sinks, max_nodes + sinks, max_edges


def mirror_dense_pool_static(P, graph_mask, parent_counts, K, drop_diagonal, n_cap_out, e_cap, sinks, sink_degree):
    P = np.asarray(P, np.float32).reshape(-1, K)
    mask = np.asarray(graph_mask).astype(bool)
    B = mask.shape[0]
    assert P.shape[0] == B * K and n_cap_out >= B * K + sinks and sinks * sink_degree >= e_cap
    m_rows = n_cap_out - sinks
    live_before = np.concatenate([[0], np.cumsum(mask)]).astype(np.int64)
    m_live = int(live_before[-1]) * K
    pooled_row_ptr = np.concatenate([live_before[:B] * K, [m_live, n_cap_out]]).astype(np.int32)
    node_index = np.full(n_cap_out, -1, np.int32)
    ngi = np.full(n_cap_out, B, np.int32)
    node_map = np.full(B * K, -1, np.int32)
    rows, cols, src, egi = [], [], [], []
    for g in np.flatnonzero(mask):
        p0 = int(pooled_row_ptr[g])
        node_index[p0:p0 + K] = g * K + np.arange(K)
        ngi[p0:p0 + K] = g
        node_map[g * K:(g + 1) * K] = p0 + np.arange(K)
        keep = P[g * K:(g + 1) * K] != np.float32(0.0)          # -0.0 is no edge, a NaN is one
        if drop_diagonal:
            keep &= ~np.eye(K, dtype=bool)
        c1, c2 = np.nonzero(keep)                                # row-major
        rows.append(p0 + c1)
        cols.append(p0 + c2)
        src.append((g * K + c1) * K + c2)
        egi.append(np.full(c1.shape[0], g))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)      # noqa: E731
    rows, cols, src, egi = cat(rows), cat(cols), cat(src), cat(egi)
    e_live = rows.shape[0]
    assert e_live <= e_cap
    q = np.arange(e_live, e_cap)
    sink = m_rows + (q - e_live) // sink_degree
    edge_index = np.stack([np.concatenate([rows, sink]), np.concatenate([cols, sink])]).astype(np.int32)
    # the two plans, in the closed forms of the header (no sort): rows [m_live, m_rows] start at e_live, sink t at
    # e_live + min(e_cap - e_live, t d); the list is sorted by row, so the plan by row is the list itself; the plan by column
    # holds a slot's entries inside the slot's own edge range in column-major order; the padded tail is the identity
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
            for g in np.flatnonzero(mask):
                n = int((egi == g).sum())                        # the slot's edges are [at, at + n) of the list
                c1, c2 = rows[at:at + n] - pooled_row_ptr[g], cols[at:at + n] - pooled_row_ptr[g]
                perm[at:at + n] = at + np.lexsort((c1, c2))      # by column, then by row
                at += n
        col = np.concatenate([other, sink])[perm]
        plans.append((row_ptr.astype(np.int32), col.astype(np.int32), perm.astype(np.int32)))
    pc = np.asarray(parent_counts, np.int32)
    return dict(plan=plans[0], plan_t=plans[1],
pooled_row_ptr=pooled_row_ptr, node_index=node_index, node_graph_index=ngi, node_map=node_map,
                edge_index=edge_index, edge_src=np.concatenate([src, np.full(q.shape[0], -1)]).astype(np.int32),
                edge_graph_index=np.concatenate([egi, np.full(q.shape[0], B)]).astype(np.int32),
                counts=np.asarray([pc[0], m_live, e_live, pc[3]], np.int32), e_live=e_live, m_live=m_live)


def mirror_pooled_weight(P, edge_src):
    """where(edge_src >= 0, P.flat[edge_src], 1.0)."""
    flat = np.asarray(P, np.float32).reshape(-1)
    src = np.asarray(edge_src)
    if flat.size == 0:
        return np.ones(src.shape[0], np.float32)
    return np.where(src >= 0, flat[np.maximum(src, 0)], np.float32(1.0)).astype(np.float32)
