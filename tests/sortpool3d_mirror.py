# coding=utf-8
"""numpy mirror of tfgx_segment_rows_3d_f32 (include/tfgx_rows3d.h) and of what is built on it: utils.convert_x_to_3d
(tf_geometric/utils/graph_utils.py:215-249) and nn.sort_pool_3d (nn/pool/sort_pool.py:7-35 followed by convert_x_to_3d), stated
from the reference's rules:

  grouping : the nodes are grouped by source, stable (tf.argsort(stable=True)); a node's slot is its position in its group;
  sort mode: within a group the nodes are ordered by the sort column DESCENDING (topk_pool.py: tf.argsort is top_k underneath:
             the lower index wins a tie, -0.0 == +0.0 — the 32-bit key of tfgx_segment_topk, tests/sagpool_static_mirror.py);
  shape    : [G, k, F], groups longer than k cut off, the rest exact zeros.

Beside `out` the mirror gives the kernel's two index outputs: slot_node [G * k] (the node of a slot, or -1) and node_slot [n]
(the slot of a node, or -1), and its flag word (a graph above the LDS cap of the sort mode keeps no node)."""
import numpy as np

from sagpool_static_mirror import MAX_GRAPH_NODES, TOO_LONG, descending_bits


def graph_plan(ids, G):
    """(seg_ptr [G + 1], seg_node [n]): the CSR over graphs, nodes in stable order."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    seg_node = np.argsort(ids, kind="stable").astype(np.int32)
    seg_ptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=G)[:G])]).astype(np.int32)
    return seg_ptr, seg_node


def mirror_rows_3d(x, seg_ptr, seg_node, G, k, sort_col=None, cap=MAX_GRAPH_NODES):
    """(out [G * k, F], slot_node [G * k], node_slot [n_rows], flags) of one call; seg_node None = the identity."""
    x = np.asarray(x, dtype=np.float32)
    n_rows, F = x.shape
    out = np.zeros((G * k, F), dtype=np.float32)
    slot_node = np.full(G * k, -1, dtype=np.int32)
    node_slot = np.full(n_rows, -1, dtype=np.int32)
    flags = 0
    for g in range(G):
        pos = np.arange(int(seg_ptr[g]), int(seg_ptr[g + 1]))
        nodes = pos if seg_node is None else np.asarray(seg_node)[pos]
        if sort_col is not None:
            if nodes.size > cap:
                flags |= TOO_LONG
                continue
            key = (descending_bits(x[nodes, sort_col]).astype(np.uint64) << np.uint64(32)) | np.arange(nodes.size, dtype=np.uint64)
            nodes = nodes[np.argsort(key, kind="stable")]
        m = min(nodes.size, k)
        out[g * k:g * k + m] = x[nodes[:m]]
        slot_node[g * k:g * k + m] = nodes[:m]
        node_slot[nodes[:m]] = g * k + np.arange(m)
    return out, slot_node, node_slot, flags


def mirror_backward(d_out, node_slot):
    """dx [n_rows, F]: row n is d_out's row node_slot[n], or zeros."""
    d_out = np.asarray(d_out, dtype=np.float32)
    d_out = d_out.reshape(-1, d_out.shape[-1])
    dx = np.zeros((node_slot.shape[0], d_out.shape[1]), dtype=np.float32)
    live = node_slot >= 0
    dx[live] = d_out[node_slot[live]]
    return dx


def _shape(ids, k, pad, num_sources):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    G = int(ids.max()) + 1 if num_sources is None else int(num_sources)
    largest = int(np.bincount(ids, minlength=max(G, 1)).max()) if ids.size else 0
    if k is None:
        k = largest
    elif k > largest and not pad:
        k = largest
    return ids, G, int(k)


def mirror_convert_x_to_3d(x, source_index, k=None, pad=True, num_sources=None, with_index=False):
    ids, G, k = _shape(source_index, k, pad, num_sources)
    seg_ptr, seg_node = graph_plan(ids, G)
    out, slot_node, node_slot, _ = mirror_rows_3d(x, seg_ptr, seg_node, G, k)
    out = out.reshape(G, k, -1)
    return (out, slot_node, node_slot) if with_index else out


def mirror_sort_pool_3d(x, node_graph_index, k, sort_index=-1, num_graphs=None, with_index=False, cap=MAX_GRAPH_NODES):
    x = np.asarray(x, dtype=np.float32)
    ids, G, _ = _shape(node_graph_index, k, True, num_graphs)
    seg_ptr, seg_node = graph_plan(ids, G)
    out, slot_node, node_slot, flags = mirror_rows_3d(x, seg_ptr, seg_node, G, k, sort_col=sort_index % x.shape[1], cap=cap)
    out = out.reshape(G, k, -1)
    return (out, slot_node, node_slot, flags) if with_index else out
