# coding=utf-8
"""numpy mirror of one fixed-shape SAGPool level (include/tfgx_pool_static.h; tf_geometric_amd.nn.sag_pool_static), stated from
the reference's rules:

  selection (tf_geometric/nn/pool/topk_pool.py:6-87): per source graph, node_k = min(k, count) or ceil(float32(count) * ratio)
      (:62-71), the scores argsorted DESCENDING (tf.argsort is top_k underneath: the lower index wins a tie, -0.0 == +0.0), the
      first node_k of every graph kept, graphs in ascending order;
  induced subgraph (tf_geometric/data/graph.py:276-359): an edge is kept iff both endpoints are, kept edges stay in their
      order and are renumbered by position in the kept-node list; edge attributes and node_graph_index are gathered.

Around that live part sits the padding of include/tfgx_collate_static.h: dead rows are zero and belong to graph B, the padded
edges are unit self-loops on the P sink rows, the plans' tail is the identity.  The plans are ASSEMBLED the way the kernels do
it (pooled row j = the kept part of parent row node_index[j] of the parent's plan); tests/test_pool_static_abi.py shows them to
be the stable sorts of the emitted lists.

A parent is the dict mirror_collate_static (tests/test_collate_static_abi.py) returns; the pooled dict has the same keys, so a
second level pools the first."""
import fractions
import math

import numpy as np

CLAMPED, TOO_LONG = 4, 8
MAX_GRAPH_NODES = 4096


def descending_bits(score):
    """uint32 keys whose ASCENDING order is the DESCENDING float order, -0.0 == +0.0 (the radix key of tfgx_segment_topk)."""
    f = np.array(score, dtype=np.float32).reshape(-1)
    f[f == 0.0] = 0.0
    u = f.view(np.uint32)
    u = np.where((u >> np.uint32(31)) != 0, u ^ np.uint32(0xFFFFFFFF), u ^ np.uint32(0x80000000))
    return (~u).astype(np.uint32)


def node_k(n, k=None, ratio=None):
    """topk_pool.py:62-71, with ratio > 1 held to n (the reference would select its padding columns)."""
    if k is not None:
        return min(int(k), int(n))
    return min(int(n), int(np.ceil(np.float32(n) * np.float32(ratio))))


def mirror_pooled_capacities(max_nodes, B, k=None, ratio=None):
    """m_max of StaticBatchGraph.pooled_capacities, evaluated exactly."""
    if k is not None:
        return min(int(max_nodes), B * int(k))
    bound = fractions.Fraction(float(np.float32(ratio))) * int(max_nodes) * (1 + fractions.Fraction(1, 1 << 22))
    return min(int(max_nodes), math.ceil(bound) + B)


def mirror_topk_static(graph_row_ptr, score, B, sinks, k=None, ratio=None, m_max=None, parent_counts=(0, 0, 0, 0)):
    """dict(node_index [n_cap'], node_map [n_cap], pooled_row_ptr [B + 2], node_graph_index [n_cap'], counts [4], m_max)."""
    grp = np.asarray(graph_row_ptr, dtype=np.int64)
    n_live, n_cap = int(grp[B]), int(grp[B + 1])
    if m_max is None:
        m_max = mirror_pooled_capacities(n_cap - sinks, B, k, ratio)
    n_cap_out = m_max + sinks
    score = np.asarray(score, dtype=np.float32).reshape(-1)
    assert score.shape[0] == n_cap
    kept, counts_g, flags = [], [], int(parent_counts[3])
    for g in range(B):
        r0, r1 = int(grp[g]), int(grp[g + 1])
        if r1 - r0 > MAX_GRAPH_NODES:
            flags |= TOO_LONG
            counts_g.append(0)
            continue
        order = np.argsort(descending_bits(score[r0:r1]), kind="stable")
        kg = node_k(r1 - r0, k, ratio)
        kept.append(r0 + order[:kg])
        counts_g.append(kg)
    kept = np.concatenate(kept).astype(np.int32) if kept else np.zeros(0, np.int32)
    m_live = kept.shape[0]
    assert m_live <= m_max, "the capacity bound"
    node_index = np.concatenate([kept, np.full(n_cap_out - m_live, -1, np.int32)]).astype(np.int32)
    node_map = np.full(n_cap, -1, np.int32)
    node_map[kept] = np.arange(m_live, dtype=np.int32)
    prp = np.concatenate([[0], np.cumsum(counts_g), [n_cap_out]]).astype(np.int32)
    ngi = np.concatenate([np.repeat(np.arange(B, dtype=np.int32), counts_g), np.full(n_cap_out - m_live, B, np.int32)]).astype(np.int32)
    assert n_live <= n_cap - sinks and (node_map[n_live:] == -1).all()
    return {"node_index": node_index, "node_map": node_map, "pooled_row_ptr": prp, "node_graph_index": ngi,
            "counts": np.asarray([parent_counts[0], m_live, 0, flags], dtype=np.int32), "m_max": m_max, "m_live": m_live}


def mirror_sag_pool_static(parent, B, sink_degree, score, k=None, ratio=None, x=None, scale=None, m_max=None):
    """The pooled dict of `parent` (see the module docstring) for the node scores `score` [n_cap]: the keys of
    mirror_collate_static plus node_index, node_map, edge_id and pooled_row_ptr.  x' = (x * scale)[node_index] in float32 when
    `x` is given (scale = the activated score, default: score), zero on the dead rows."""
    P, n_cap, e_cap = parent["sinks"], parent["n_cap"], parent["e_cap"]
    sel = mirror_topk_static(parent["graph_plan"][0], score, B, P, k, ratio, m_max, parent["counts"])
    node_index, node_map, m_live, m_max = sel["node_index"], sel["node_map"], sel["m_live"], sel["m_max"]
    n_out = m_max + P
    ei = np.asarray(parent["edge_index"]).astype(np.int64)
    keep = (node_map[ei[0]] >= 0) & (node_map[ei[1]] >= 0)
    edge_id = np.nonzero(keep)[0].astype(np.int32)
    e_kept = edge_id.shape[0]
    tail = np.arange(e_cap - e_kept)
    sink_of = (n_out - P + tail // sink_degree).astype(np.int32)
    assert e_kept == e_cap or sink_of.max() < n_out
    out = {"edge_index": np.concatenate([node_map[ei[:, keep]], np.stack([sink_of, sink_of])], axis=1).astype(np.int32),
           "edge_weight": np.concatenate([parent["edge_weight"][keep], np.ones(e_cap - e_kept, np.float32)]).astype(np.float32),
           "edge_graph_index": np.concatenate([parent["edge_graph_index"][keep], np.full(e_cap - e_kept, B, np.int32)]).astype(np.int32),
           "edge_id": np.concatenate([edge_id, np.full(e_cap - e_kept, -1, np.int32)]).astype(np.int32),
           "node_graph_index": sel["node_graph_index"], "node_index": node_index, "node_map": node_map,
           "pooled_row_ptr": sel["pooled_row_ptr"], "graph_mask": parent["graph_mask"],
           "counts": np.asarray([parent["counts"][0], m_live, e_kept, sel["counts"][3]], dtype=np.int32),
           "n_live": m_live, "e_live": e_kept, "sinks": P, "n_cap": n_out, "e_cap": e_cap}
    if x is not None:
        scale = score if scale is None else scale
        scaled = np.asarray(x, np.float32) * np.asarray(scale, np.float32).reshape(-1, 1)
        out["x"] = np.where(node_index[:, None] >= 0, scaled[np.maximum(node_index, 0)], np.float32(0.0)).astype(np.float32)
    # the plans, assembled: pooled row j = the kept part of parent row node_index[j], walked in CSR order
    rank = np.full(e_cap, -1, np.int32)
    rank[edge_id] = np.arange(e_kept, dtype=np.int32)
    dead_rows = np.arange(m_live, n_out + 1)
    dead_ptr = e_kept + np.minimum(e_cap - e_kept, np.maximum(dead_rows - (n_out - P), 0) * sink_degree)
    for key in ("plan", "plan_t"):
        p_row_ptr, p_col, p_perm = parent[key]
        cols, perms, cnt = [], [], []
        for j in range(m_live):
            o = int(node_index[j])
            seg = slice(int(p_row_ptr[o]), int(p_row_ptr[o + 1]))
            nc = node_map[p_col[seg]]
            cols.append(nc[nc >= 0])
            perms.append(rank[p_perm[seg][nc >= 0]])
            cnt.append(int((nc >= 0).sum()))
        live_ptr = np.concatenate([[0], np.cumsum(cnt)])[:m_live]
        assert sum(cnt) == e_kept
        out[key] = (np.concatenate([live_ptr, dead_ptr]).astype(np.int32),
                    np.concatenate(cols + [sink_of]).astype(np.int32), np.concatenate(perms + [e_kept + tail]).astype(np.int32))
    nodes = np.arange(n_out, dtype=np.int32)
    out["graph_plan"] = (sel["pooled_row_ptr"], nodes, nodes)
    return out
