# coding=utf-8
"""SAGPool (reference: tf_geometric/nn/pool/sag_pool.py:7-45): score the nodes with a GNN, keep the top ones of every
graph (topk_pool on the RAW score), scale the kept rows by score_activation(score) and take the induced subgraph.
Kernels: tfgx_segment_topk, tfgx_induced_subgraph_{count,emit} (the pooled CSR plan derived from the parent's, no sort),
tfgx_gather_scale_rows_f32 (+ its backward), tfgx_permute_rows_f32 / tfgx_gather_i32 for edge weights / graph ids."""
import numpy as np
import torch

from ... import _lib as L
from ...plan import attach_plan, attached_plan
from ...utils.subgraph import pool_graph, parent_plan_of, refuse_capture
from .topk_pool import topk_pool


def _with_plan(edge_index, plan):
    """edge_index as handed to the score GNN: a tensor carrying the parent plan (an alias, so the caller's tensor object is
    left alone), so the GNN does not sort the edge list again.  numpy stays as given."""
    if not isinstance(edge_index, torch.Tensor) or attached_plan(edge_index) is not None:
        return edge_index
    alias = edge_index.view(edge_index.shape)      # shares the caller's storage AND version counter
    return attach_plan(alias, plan)


def sag_pool(x, edge_index, edge_weight, node_graph_index, score_gnn, k=None, ratio=None, score_activation=None,
             training=None, cache=None):
    """
    Functional API for SAGPool (same arguments as the reference).

    :param x: [num_nodes, num_features] node features
    :param edge_index: [2, num_edges]
    :param edge_weight: [num_edges] or None
    :param node_graph_index: [num_nodes] graph id of every node
    :param score_gnn: [x, edge_index, edge_weight] => node_score ([num_nodes, 1])
    :param k / ratio: keep top k (or num_nodes * ratio) nodes of every graph
    :param score_activation: applied to node_score AFTER the ranking, before it multiplies the features
    :param cache: handed to score_gnn when given (its CSR plan is also the parent plan of the pooled graph)
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]
    """
    refuse_capture("sag_pool")
    L.require_gpu()
    n = int(np.shape(x)[0])
    plan = parent_plan_of(edge_index, n, cache) if isinstance(edge_index, torch.Tensor) else None
    gnn_edge_index = _with_plan(edge_index, plan) if plan is not None else edge_index
    if cache is None:
        node_score = score_gnn([x, gnn_edge_index, edge_weight], training=training)                  # :29-32
    else:
        node_score = score_gnn([x, gnn_edge_index, edge_weight], training=training, cache=cache)
    ngi = L.as_i32(node_graph_index)
    topk_node_index = topk_pool(ngi, node_score, k=k, ratio=ratio)                                  # :34
    if score_activation is not None:
        node_score = score_activation(node_score)                                                   # :36-37
    return list(pool_graph(x, edge_index, edge_weight, node_graph_index, topk_node_index, n, score=node_score,
                           plan=plan))                                                              # :39-45
