# coding=utf-8
"""SortPool (reference: tf_geometric/nn/pool/sort_pool.py:7-35): rank the nodes of every graph by one feature column,
keep the top ones and take the induced subgraph (the same kernels as sag_pool, the row gather without a multiplier)."""
import numpy as np
import torch

from ... import _lib as L
from ...plan import attached_plan
from ...utils.subgraph import pool_graph, refuse_capture
from .topk_pool import topk_pool


def sort_pool(x, edge_index, edge_weight, node_graph_index, k=None, ratio=None, sort_index=-1, training=None):
    """
    Functional API for SortPool "An End-to-End Deep Learning Architecture for Graph Classification".

    :param sort_index: the column of x that ranks the nodes
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]; x stays numpy when given as numpy
    """
    refuse_capture("sort_pool")
    L.require_gpu()
    xt = L.as_f32(x)
    score = xt.detach()[:, sort_index]                                                              # :26
    topk_node_index = topk_pool(L.as_i32(node_graph_index), score, k=k, ratio=ratio)                # :27
    plan = attached_plan(edge_index)
    return list(pool_graph(xt, edge_index, edge_weight, node_graph_index, topk_node_index, int(np.shape(x)[0]),
                           plan=plan, x_numpy=not isinstance(x, torch.Tensor)))                     # :29-35
