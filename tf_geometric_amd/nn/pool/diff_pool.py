# coding=utf-8
"""DiffPool (reference: tf_geometric/nn/pool/diff_pool.py:8-105): coarsen every graph of a batch by a DENSE assignment of its
nodes to num_clusters clusters: pooled adjacency S^T A S, pooled features S^T h.

The reference turns the dense assignment into a sparse [N, G K] one and goes through cluster_pool's dense [N, N] adjacency.
Here the block structure is used directly: node n of graph g has clusters [g K, (g + 1) K) only, so every product is a
per-graph [K, n_g] x [n_g, W] product, ragged in n_g — one tfgx_segment_gram_f32 launch pair each (include/tfgx_seggram.h):
    AS = A S             the existing aggregation kernel over [N, K] rows, on the cached CSR plan
    P  = S_g^T (A S)_g   -> [G K, K]: the diagonal blocks of the pooled adjacency
    pooled_x = S_g^T h_g -> [G K, F]
No [N, N], [G K, G K] or padded [G, n_max, K] tensor is made; everything is differentiable in S, h and (DiffPool) the edge
weights.  An edge between two graphs would put an entry outside the diagonal blocks: it is refused."""
import numpy as np
import torch

from ... import _lib as L
from ... import autograd as AG
from ...plan import CsrPlan, attach_plan, attached_plan, segment_reduce
from ...utils.subgraph import refuse_capture
from .common_pool import _graph_plan

CACHE_KEY_DENSE_POOL = "tfgx_dense_pool"


def _same_storage(key, t):
    return key[0].data_ptr() == t.data_ptr() and key[0].shape == t.shape and key[1] == t._version


class _Prepared(object):
    """What depends on the edge LIST and the graph ids only: both as int32 device tensors (kept alive with the version
    counters they had), the CSR plan of the list, the CSR over graphs, and the fact that no edge joins two graphs."""

    def __init__(self, ei, ids, plan, graph_plan, num_graphs):
        self.ei, self.ids, self.plan, self.graph_plan, self.num_graphs = ei, ids, plan, graph_plan, num_graphs
        self.keys = ((ei, ei._version), (ids, ids._version))


def _prepare(what, edge_index, node_graph_index, num_nodes, num_graphs, cache):
    """Host reads: max(node_graph_index) when num_graphs is None; on a cold cache the two plan builders (each reports bad
    indices to the host) and the verdict on cross-graph edges.  With a `cache` that saw the same int32 device tensors
    (same storage, unmodified) and the same num_graphs: none."""
    dev = L.device()
    n = int(num_nodes)
    ei = L.as_i32(edge_index, dev)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    ids = L.as_i32(node_graph_index, dev).reshape(-1)
    if int(ids.shape[0]) != n:
        raise ValueError("{}: node_graph_index has {} entries, the graph has {} nodes".format(what, int(ids.shape[0]), n))
    if num_graphs is None:
        if n == 0:
            raise ValueError("{}: num_graphs cannot be derived from an empty node_graph_index".format(what))
        num_graphs = int(ids.max().item()) + 1                             # diff_pool.py:36
    G = int(num_graphs)
    hit = None if cache is None else cache.get(CACHE_KEY_DENSE_POOL)
    if hit is not None and _same_storage(hit.keys[0], ei) and _same_storage(hit.keys[1], ids) and hit.num_graphs == G \
            and hit.plan.n_dst == n:
        return hit
    graph_plan = _graph_plan(ids, G, n, cache)
    attached = attached_plan(edge_index)          # a previous pooling layer / sampler / drop_edge handed its plan on
    plan = attached.padded_to(n, n) if attached is not None else None
    if plan is None:
        plan = CsrPlan.build(ei, n, n)            # validates the endpoints
    if int(ei.shape[1]) and bool((ids[ei[0].long()] != ids[ei[1].long()]).any().item()):
        raise ValueError("{}: edge_index holds an edge between two graphs of the batch; the pooled adjacency would leave its "
                         "diagonal blocks (cross-graph edges are not supported)".format(what))
    prep = _Prepared(ei, ids, plan, graph_plan, G)
    if cache is not None:
        cache[CACHE_KEY_DENSE_POOL] = prep
    return prep


def _check_assign(what, dense_assign, num_nodes, num_clusters):
    S = L.as_f32(dense_assign)
    if S.dim() != 2:
        raise ValueError("{}: dense_assign must be [num_nodes, num_clusters], got {}".format(what, tuple(S.shape)))
    n, K = int(S.shape[0]), int(S.shape[1])
    if num_nodes is not None and int(num_nodes) != n:
        raise ValueError("{}: num_nodes = {} but dense_assign has {} rows".format(what, int(num_nodes), n))
    if num_clusters is not None and int(num_clusters) != K:
        raise ValueError("{}: num_clusters = {} but dense_assign has {} columns".format(what, int(num_clusters), K))
    if not 1 <= K <= L.SEGGRAM_MAX_K:
        raise ValueError("{}: {} clusters per graph; the segmented product kernel serves 1 .. TFGX_SEGGRAM_MAX_K = {}".format(
            what, K, L.SEGGRAM_MAX_K))
    return S.contiguous(), n, K


def _adjacency_times(prep, M, w):
    """A M on the plan of the edge list (A[row, col] = w, duplicates add up); differentiable in M and w."""
    w_csr = AG.edge_attr_csr(prep.plan, w)
    if AG.needs_grad(M, w_csr):
        return AG.aggregate(prep.plan, M, L.SUM, w_csr=w_csr)
    return segment_reduce(prep.plan, M, L.SUM, w_csr=w_csr)


def _pooled_edges(P, G, K, drop_diagonal):
    """convert_dense_adj_to_edge of the block-diagonal matrix whose blocks are P [G K, K] (graph_utils.py:272-284): the
    entries != 0.0 in row-major order, row g K + c1, column g K + c2; without c1 == c2 when drop_diagonal
    (min_cut_pool.py:143).  One host read: the count.  The list is sorted by row, so its CSR plan is arithmetic."""
    dev = P.device
    flat = P.reshape(-1)
    keep = flat.detach() != 0.0
    if drop_diagonal:
        pos = torch.arange(G * K * K, dtype=torch.int64, device=dev)
        keep = keep & ((pos // K) % K != pos % K)
    idx = torch.nonzero(keep).flatten()
    row = idx // K
    col = ((row // K) * K + idx % K).to(torch.int32)
    pei = torch.stack([row.to(torch.int32), col]).contiguous()
    row_ptr = torch.zeros(G * K + 1, dtype=torch.int32, device=dev)
    row_ptr[1:] = torch.cumsum(keep.reshape(G * K, K).sum(dim=1), dim=0)
    plan = CsrPlan.from_sorted(row_ptr, pei[1], G * K, edge_index=pei)
    return attach_plan(pei, plan), flat[idx]


def _coarsen(what, x, edge_index, adjacency_weight, node_graph_index, S, n, K, num_graphs, cache, drop_diagonal):
    prep = _prepare(what, edge_index, node_graph_index, n, num_graphs, cache)
    G, dev = prep.num_graphs, S.device
    E = int(prep.ei.shape[1])
    w = None
    if adjacency_weight is not None:
        w = L.as_f32(adjacency_weight, dev).reshape(-1)
        if int(w.shape[0]) != E:
            raise ValueError("{}: edge_weight has {} entries, edge_index has {} edges".format(what, int(w.shape[0]), E))
    P = AG.segment_gram(prep.graph_plan, prep.ids, S, _adjacency_times(prep, S, w))            # cluster_pool.py:36
    pooled_x = None
    if x is not None:
        h = L.as_f32(x, dev)
        if h.dim() != 2 or int(h.shape[0]) != n:
            raise ValueError("{}: x must be [{}, F], got {}".format(what, n, tuple(h.shape)))
        pooled_x = AG.segment_gram(prep.graph_plan, prep.ids, S, h)                            # cluster_pool.py:42
    pooled_edge_index, pooled_edge_weight = _pooled_edges(P, G, K, drop_diagonal)
    pooled_ngi = torch.arange(G, dtype=torch.int32, device=dev).repeat_interleave(K)          # diff_pool.py:50
    if not isinstance(edge_index, torch.Tensor):
        pooled_edge_index = pooled_edge_index.cpu().numpy()
        pooled_edge_weight = pooled_edge_weight.detach().cpu().numpy()
    if not isinstance(node_graph_index, torch.Tensor):
        pooled_ngi = pooled_ngi.cpu().numpy()
    return pooled_x, pooled_edge_index, pooled_edge_weight, pooled_ngi


def diff_pool_coarsen(x, edge_index, edge_weight, node_graph_index, dense_assign,
                      num_nodes=None, num_clusters=None, num_graphs=None, cache=None):
    """
    Coarsening method for DiffPool (the reference's arguments and order, plus cache=).

    :param x: [num_nodes, num_features] node features, or None
    :param edge_index: [2, num_edges]; no edge may join two graphs (ValueError)
    :param edge_weight: [num_edges] or None (ones)
    :param node_graph_index: [num_nodes] graph id of every node (any order)
    :param dense_assign: [num_nodes, num_clusters] assignment of every node to the clusters of ITS graph,
        num_clusters <= TFGX_SEGGRAM_MAX_K
    :param num_nodes / num_clusters: checked against dense_assign when given
    :param num_graphs: avoids one host read (max(node_graph_index) + 1)
    :param cache: a dict that keeps the CSR plan of the edge list, the CSR over graphs and the verdict on cross-graph edges
        for the same int32 device tensors edge_index / node_graph_index.  Different graphs must not share a cache dict.
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]: pooled_x [G K, F] = S_g^T x_g; the
        entries != 0.0 of the block-diagonal S^T A S in row-major order (int32 [2, nnz], float32 [nnz]), carrying their CSR
        plan for the next layer; arange(G) repeated K times.  numpy in -> numpy out for the edge list and the graph ids.

    Differentiable in x, dense_assign and edge_weight.  Not capturable in a hipGraph (the pooled edge count is read back).
    """
    L.require_gpu()
    refuse_capture("diff_pool_coarsen")
    S, n, K = _check_assign("diff_pool_coarsen", dense_assign, num_nodes, num_clusters)
    return _coarsen("diff_pool_coarsen", x, edge_index, edge_weight, node_graph_index, S, n, K, num_graphs, cache, False)


def _call_gnn(gnn, inputs, training, cache):
    if cache is None:
        return gnn(inputs, training=training)                              # diff_pool.py:85-90
    return gnn(inputs, training=training, cache=cache)


def diff_pool(x, edge_index, edge_weight, node_graph_index,
              feature_gnn, assign_gnn,
              num_clusters, bias=None, activation=None, cache=None, training=None, num_graphs=None):
    """
    Functional API for DiffPool: "Hierarchical graph representation learning with differentiable pooling" (the reference's
    arguments and order, plus num_graphs=).

    :param feature_gnn / assign_gnn: callables [x, edge_index, edge_weight] -> [num_nodes, F'] / [num_nodes, num_clusters]
        (called with training= and, when a cache is given, cache=)
    :param num_clusters: clusters per graph, <= TFGX_SEGGRAM_MAX_K
    :param bias: [F'] or None; activation: applied to the pooled features
    :param cache: see diff_pool_coarsen; also handed to the two GNNs
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]
    """
    L.require_gpu()
    refuse_capture("diff_pool")
    x = L.as_f32(x)
    if edge_weight is None:                                                # :78-80
        edge_weight = torch.ones(int(np.shape(edge_index)[-1]), dtype=torch.float32, device=x.device)
    assign_logits = _call_gnn(assign_gnn, [x, edge_index, edge_weight], training, cache)
    h = _call_gnn(feature_gnn, [x, edge_index, edge_weight], training, cache)
    assign_probs = torch.softmax(L.as_f32(assign_logits), dim=-1)         # :92
    S, n, K = _check_assign("diff_pool", assign_probs, int(x.shape[0]), num_clusters)
    pooled_h, pooled_edge_index, pooled_edge_weight, pooled_ngi = _coarsen(
        "diff_pool", h, edge_index, edge_weight, node_graph_index, S, n, K, num_graphs, cache, False)
    if bias is not None:
        pooled_h = AG.bias_add(pooled_h, L.as_f32(bias, pooled_h.device))  # :99-100
    if activation is not None:
        pooled_h = activation(pooled_h)
    return [pooled_h, pooled_edge_index, pooled_edge_weight, pooled_ngi]
