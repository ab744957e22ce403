# coding=utf-8
"""MinCutPool (reference: tf_geometric/nn/pool/min_cut_pool.py:18-232): DiffPool's coarsening on the normalised adjacency
D^-1/2 A D^-1/2 without the pooled self-loops, and two unsupervised losses of the assignment:
    cut  = mean_g( -tr(S_g^T A S_g) / (tr(S_g^T D S_g) + 1e-8) )
    orth = mean_g || S_g^T S_g / (||S_g^T S_g||_F + 1e-8) - I / sqrt(K) ||_F
Every product is a per-graph S_g^T Y_g on the segmented kernel of include/tfgx_seggram.h (nn/pool/diff_pool.py); what
follows the products is [G, K, K]-sized torch.  The reference densifies A ([N, N]) three times for the losses alone."""
import numpy as np
import torch

from ... import _lib as L
from ... import autograd as AG
from ...utils import adj_norm_edge
from ...utils.subgraph import refuse_capture
from ..conv.propagation import _refuse_trainable_edge_weight
from .diff_pool import _adjacency_times, _call_gnn, _check_assign, _coarsen, _prepare


def _ones_like_edges(edge_index, dev):
    return torch.ones(int(np.shape(edge_index)[-1]), dtype=torch.float32, device=dev)


def min_cut_pool_compute_losses(edge_index, edge_weight, node_graph_index, dense_assign, normed_edge_weight=None,
                                cache=None, num_graphs=None):
    """(cut_loss, orth_loss), two scalars, as min_cut_pool.py:18-90 (the reference's arguments and order, plus num_graphs=).
    normed_edge_weight=None normalises edge_weight with adj_norm_edge(add_self_loop=False); the degree is the row sum of the
    NORMALISED weights (:29).  Differentiable in dense_assign (and in a normed_edge_weight that is passed in); an edge_weight
    that requires grad raises NotImplementedError, because adj_norm_edge is raw kernel launches."""
    L.require_gpu()
    refuse_capture("min_cut_pool_compute_losses")
    S, n, K = _check_assign("min_cut_pool_compute_losses", dense_assign, None, None)
    dev = S.device
    if normed_edge_weight is None:
        _refuse_trainable_edge_weight(edge_weight, "min_cut_pool_compute_losses")
        _, normed_edge_weight = adj_norm_edge(edge_index, n, edge_weight, add_self_loop=False, cache=cache)     # :25-26
    prep = _prepare("min_cut_pool_compute_losses", edge_index, node_graph_index, n, num_graphs, cache)
    G = prep.num_graphs
    w = L.as_f32(normed_edge_weight, dev).reshape(-1)
    degree = _adjacency_times(prep, torch.ones((n, 1), dtype=torch.float32, device=dev), w)                     # :29
    blocks = lambda Y: AG.segment_gram(prep.graph_plan, prep.ids, S, Y).reshape(G, K, K)                        # noqa: E731
    trace = lambda M: torch.diagonal(M, dim1=1, dim2=2).sum(dim=-1)                                             # noqa: E731
    intra_edge_sum = trace(blocks(_adjacency_times(prep, S, w)))                                                # :64
    all_edge_sum = trace(blocks(degree * S))                                                                    # :66
    cut_loss = torch.mean(-intra_edge_sum / (all_edge_sum + 1e-8))                                              # :69
    STS = blocks(S)                                                                                             # :76-80
    norm_STS = torch.sqrt(torch.sum(STS * STS, dim=(-2, -1), keepdim=True))                                     # :82
    normed_STS = STS / (norm_STS + 1e-8)
    eye = torch.eye(K, dtype=torch.float32, device=dev) / torch.sqrt(torch.tensor(float(K), dtype=torch.float32, device=dev))
    deviation = normed_STS - eye                                                                                # :86-87
    orth_loss = torch.mean(torch.sqrt(torch.sum(deviation * deviation, dim=(-2, -1))))                          # :89
    return cut_loss, orth_loss


def min_cut_pool_coarsen(x, edge_index, edge_weight, node_graph_index, dense_assign,
                         num_nodes=None, num_clusters=None, num_graphs=None, normed_edge_weight=None, cache=None):
    """
    Coarsening method for MinCutPool (the reference's arguments and order): diff_pool_coarsen on the normalised edge weights,
    then the pooled self-loops are removed (min_cut_pool.py:127-143).

    :param normed_edge_weight: [num_edges] or None: adj_norm_edge(edge_index, num_nodes, edge_weight, cache=cache)
    :param cache: as diff_pool_coarsen; also adj_norm_edge's
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]; the edge list holds the entries
        != 0.0 of S^T A S with c1 != c2 and carries its CSR plan.

    Differentiable in x, dense_assign and a normed_edge_weight that is passed in; an edge_weight that requires grad raises
    NotImplementedError when it has to be normalised here.
    """
    L.require_gpu()
    refuse_capture("min_cut_pool_coarsen")
    S, n, K = _check_assign("min_cut_pool_coarsen", dense_assign, num_nodes, num_clusters)
    if normed_edge_weight is None:
        _refuse_trainable_edge_weight(edge_weight, "min_cut_pool_coarsen")
        _, normed_edge_weight = adj_norm_edge(edge_index, n, edge_weight, cache=cache)                          # :127-128
    return _coarsen("min_cut_pool_coarsen", x, edge_index, normed_edge_weight, node_graph_index, S, n, K, num_graphs, cache,
                    True)


def min_cut_pool(x, edge_index, edge_weight, node_graph_index,
                 feature_gnn, assign_gnn,
                 num_clusters, bias=None, activation=None,
                 gnn_use_normed_edge=True,
                 return_loss_func=False, return_losses=False,
                 cache=None, training=None, num_graphs=None):
    """
    Functional API for MinCutPool: "Spectral Clustering with Graph Neural Networks for Graph Pooling" (the reference's
    arguments and order, plus num_graphs=).

    :param feature_gnn / assign_gnn: callables [x, edge_index, edge_weight] -> [num_nodes, F'] / [num_nodes, num_clusters]
    :param gnn_use_normed_edge: hand the two GNNs the normalised edge weights
    :param return_loss_func: return (outputs, loss_func); loss_func() -> (cut_loss, orth_loss)
    :param return_losses: return (outputs, (cut_loss, orth_loss))
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]

    An edge_weight that requires grad raises NotImplementedError (the normalisation is raw kernel launches).
    """
    if return_loss_func and return_losses:
        raise ValueError("return_loss_func and return_losses cannot be set to True at the same time")          # :179-180
    L.require_gpu()
    refuse_capture("min_cut_pool")
    _refuse_trainable_edge_weight(edge_weight, "min_cut_pool")
    x = L.as_f32(x)
    n = int(x.shape[0])
    if edge_weight is None:
        edge_weight = _ones_like_edges(edge_index, x.device)                                                    # :182-184
    _, normed_edge_weight = adj_norm_edge(edge_index, n, edge_weight, add_self_loop=False, cache=cache)         # :190
    gnn_edge_weight = normed_edge_weight if gnn_use_normed_edge else edge_weight
    assign_logits = _call_gnn(assign_gnn, [x, edge_index, gnn_edge_weight], training, cache)
    h = _call_gnn(feature_gnn, [x, edge_index, gnn_edge_weight], training, cache)
    assign_probs = torch.softmax(L.as_f32(assign_logits), dim=-1)                                              # :204
    S, n, K = _check_assign("min_cut_pool", assign_probs, n, num_clusters)
    pooled_h, pooled_edge_index, pooled_edge_weight, pooled_ngi = _coarsen(
        "min_cut_pool", h, edge_index, normed_edge_weight, node_graph_index, S, n, K, num_graphs, cache, True)
    if bias is not None:
        pooled_h = AG.bias_add(pooled_h, L.as_f32(bias, pooled_h.device))
    if activation is not None:
        pooled_h = activation(pooled_h)
    outputs = [pooled_h, pooled_edge_index, pooled_edge_weight, pooled_ngi]
    if not (return_loss_func or return_losses):
        return outputs
    G = int(np.shape(pooled_ngi)[0]) // K

    def loss_func():
        return min_cut_pool_compute_losses(edge_index, edge_weight, node_graph_index, S,
                                           normed_edge_weight=normed_edge_weight, cache=cache, num_graphs=G)   # :222-224

    if return_loss_func:
        return outputs, loss_func
    return outputs, loss_func()
