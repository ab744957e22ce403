# coding=utf-8
"""ASAP: Adaptive Structure Aware Pooling (reference: tf_geometric/nn/pool/asap.py:19-131).

Every node is a candidate cluster made of its 1-hop neighbourhood: a GCN gives attention features, a master query (the
neighbourhood's maximum) scores every member, a softmax over the neighbourhood weights the members' features into the cluster
feature, LEConv scores the clusters, the top ones of every graph are kept, and the kept clusters are joined by S^T A S.

Two repairs against the reference as written, both needed for it to run at all on its own current code: its gcn() call uses
the argument order from before SparseMatrix (asap.py:54), and it hands cluster_pool [cluster; node] where cluster_pool reads
[node; cluster] (asap.py:110-123).  Everything else is the reference's arithmetic.

Kernels: tfgx_asap_attend_f32 (scores, softmax, dropout and the weighted feature sum in ONE launch over the CSR plan of the
self-loop-free edge list; the self edge is implicit), tfgx_asap_attend_backward_f32, tfgx_spasp_count / _emit / _reduce (the
sparse S^T A S), and the existing GCN / max-aggregation / LEConv / top-k / gather-scale paths.  No [N, N], [K, K], [E, F] or
[E, 2A] tensor is made."""
import numpy as np
import torch

from ... import _lib as L
from ... import autograd as AG
from ...plan import CsrPlan, attach_plan, attached_plan, segment_reduce
from ...sparse import SparseMatrix
from ...utils.subgraph import refuse_capture, gather_i32
from ..conv.gcn import gcn
from ..conv.propagation import le_conv, _dense
from .cluster_pool import sparse_sas
from .topk_pool import topk_pool

CACHE_KEY_ASAP = "tfgx_asap"


class _Prepared(object):
    """What depends on the edge LIST only: the list without self-loops (an alias carrying its plan), the positions kept from
    the caller's list (None: nothing was removed), the plan and the cache dict of the attention GCN."""

    def __init__(self, edge_index, keep, plan):
        self.edge_index, self.keep, self.plan, self.gcn_cache = edge_index, keep, plan, {}
        self.num_graphs = None          # max(node_graph_index) + 1, read once


def _prepare(edge_index, ei, n):
    loops = ei[0] == ei[1]
    if int(ei.shape[1]) and bool(loops.any().item()):
        keep = torch.nonzero(~loops).flatten()
        ei0 = ei[:, keep].contiguous()
        plan = CsrPlan.build(ei0, n, n)
    else:
        keep = None
        attached = attached_plan(edge_index)          # a previous pooling layer / sampler / drop_edge handed its plan on
        plan = attached.padded_to(n, n) if attached is not None else None
        if plan is None:
            plan = CsrPlan.build(ei, n, n)
        ei0 = ei.view(ei.shape)                         # an alias: the caller's tensor object is left alone
    if plan._edge_index is None:
        plan._edge_index = ei0
    AG._transposed(plan)                                # built once here; the backward pass and S both walk it
    return _Prepared(attach_plan(ei0, plan), keep, plan)


def _assignment(plan, pw, pws, node_map):
    """S [N, K] in CSR by node for the spasp kernels: S[j, r] = the weight of edge (idx[r], j), self edges included.  The
    transposed plan already groups the edges by j; the self entry goes to the end of every row, and an entry whose attending
    row was not selected keeps cluster id -1 (the kernels skip it): no compaction, no sort, no host read."""
    pt, t2d = AG._transposed(plan)
    N, E = plan.n_dst, plan.num_edges
    dev = pw.device
    ar = torch.arange(N, dtype=torch.int64, device=dev)
    s_row_ptr = (pt.row_ptr.to(torch.int64) + torch.arange(N + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    s_col = torch.empty(E + N, dtype=torch.int32, device=dev)
    s_val = torch.empty(E + N, dtype=torch.float32, device=dev)
    pos = torch.arange(E, dtype=torch.int64, device=dev) + AG.plan_rows(pt)
    s_col[pos] = node_map[pt.col.long()]
    s_val[pos] = pw[t2d.long()]
    self_pos = pt.row_ptr[1:].to(torch.int64) + ar
    s_col[self_pos] = node_map
    s_val[self_pos] = pws
    return s_row_ptr, s_col, s_val


def _pooled_plan(row, col, row_ptr, K):
    """The pooled edge list [off-diagonal entries sorted by (row, col); then the K diagonal edges] and its CSR plan, which is
    arithmetic: row r holds its off-diagonal entries in list order and then its diagonal edge (id nnz + r), exactly where
    CsrPlan.build's stable sort by row would put them."""
    dev = row.device
    nnz = int(row.shape[0])
    ark = torch.arange(K, dtype=torch.int32, device=dev)
    pei = torch.cat([torch.stack([row, col]), torch.stack([ark, ark])], dim=1).contiguous()
    p_row_ptr = (row_ptr + torch.arange(K + 1, dtype=torch.int32, device=dev)).contiguous()
    p_col = torch.empty(nnz + K, dtype=torch.int32, device=dev)
    p_perm = torch.empty(nnz + K, dtype=torch.int32, device=dev)
    pos = torch.arange(nnz, dtype=torch.int64, device=dev) + row.long()
    p_col[pos] = col
    p_perm[pos] = torch.arange(nnz, dtype=torch.int32, device=dev)
    dpos = row_ptr[1:].long() + ark.long()
    p_col[dpos] = ark
    p_perm[dpos] = ark + nnz
    plan = CsrPlan(p_row_ptr, p_col, p_perm, K, K, nnz + K)
    plan._edge_index = pei
    return attach_plan(pei, plan)


def asap(x, edge_index, edge_weight, node_graph_index,
         attention_gcn_kernel, attention_gcn_bias,
         attention_query_kernel, attention_query_bias,
         attention_score_kernel, attention_score_bias,
         le_conv_self_kernel, le_conv_self_bias,
         le_conv_aggr_self_kernel, le_conv_aggr_self_bias,
         le_conv_aggr_neighbor_kernel, le_conv_aggr_neighbor_bias,
         k=None, ratio=None, le_conv_activation=torch.sigmoid, drop_rate=0.0, training=None, cache=None, seed=None):
    """
    Functional API for ASAP (the reference's arguments and order, plus seed=).

    :param x: [num_nodes, num_features] node features
    :param edge_index: [2, num_edges]; self-loops are removed, duplicates stay duplicates
    :param edge_weight: [num_edges] or None
    :param node_graph_index: [num_nodes] graph id of every node
    :param attention_gcn_kernel / _bias: [F, A] / [A]; attention_query_kernel / _bias: [A, A] / [A];
        attention_score_kernel / _bias: [2A, 1] / [1]
    :param le_conv_*: the six LEConv weights ([F, 1] kernels, [1] biases or None)
    :param k / ratio: keep the top k (or num_nodes * ratio) clusters of every graph
    :param le_conv_activation: applied to the kept clusters' scores before they multiply the features (None: raw score)
    :param drop_rate / training: dropout on the attention weights, by the counter-based rule tfgx_dropout_keep(seed, CSR
        position of the edge (num_edges + i for the self edge of node i), drop_rate); TensorFlow's random stream is not
        reproduced
    :param seed: the dropout seed; None draws one from torch's CPU generator
    :param cache: a dict that keeps, under "tfgx_asap", the plan of the self-loop-free edge list, its transposed plan and the
        attention GCN's normalised adjacency (which, as in the reference, includes the edge weights of the first call).
        Different graphs must not share a cache dict.
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_node_graph_index]; the pooled edge list is the
        off-diagonal entries != 0.0 of S^T A S in row-major order followed by one unit self-loop per cluster, and carries its
        CSR plan for the next layer.  numpy in -> numpy out for the edge list, its weights and the graph ids.
    """
    refuse_capture("asap")
    L.require_gpu()
    x = L.as_f32(x)
    n = int(x.shape[0])
    dev = x.device
    ei_np = not isinstance(edge_index, torch.Tensor)
    ei = L.as_i32(edge_index, dev)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    if edge_weight is not None and int(np.shape(edge_weight)[0]) != int(ei.shape[1]):
        raise ValueError("edge_weight has {} entries, edge_index has {} edges".format(int(np.shape(edge_weight)[0]),
                                                                                   int(ei.shape[1])))
    if int(np.shape(node_graph_index)[0]) != n:
        raise ValueError("node_graph_index has {} entries, the graph has {} nodes".format(int(np.shape(node_graph_index)[0]), n))
    prep = cache.get(CACHE_KEY_ASAP) if cache is not None else None
    if prep is None or prep.plan.n_dst != n:
        prep = _prepare(edge_index, ei, n)                                                           # asap.py:48
        if cache is not None:
            cache[CACHE_KEY_ASAP] = prep
    plan, ei0 = prep.plan, prep.edge_index
    w0 = None
    if edge_weight is not None:
        w0 = L.as_f32(edge_weight, dev).reshape(-1)
        if prep.keep is not None:
            w0 = w0[prep.keep]
    rate = float(drop_rate) if (training and drop_rate > 0) else 0.0
    if rate > 0.0 and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())

    h = gcn(x, SparseMatrix(ei0, w0, [n, n]), attention_gcn_kernel, attention_gcn_bias, cache=prep.gcn_cache)   # :54
    # the master query: max over the neighbourhood, the node itself included (:57-63); an empty row holds float32 lowest
    hmax = AG.aggregate(plan, h, L.MAX) if AG.needs_grad(h) else segment_reduce(plan, h, L.MAX)
    query = _dense(torch.maximum(hmax, h), attention_query_kernel, attention_query_bias)          # :65
    A = int(h.shape[1])
    ks = L.as_f32(attention_score_kernel, dev)
    if tuple(ks.shape) != (2 * A, 1):
        raise ValueError("attention_score_kernel must be [{}, 1], got {}".format(2 * A, tuple(ks.shape)))
    # concat(query_i, h_j) @ [2A, 1] = query_i @ top + h_j @ bottom: two scalars per node (:67-71)
    sq = _dense(query, ks[:A]).reshape(-1)
    sh = _dense(h, ks[A:]).reshape(-1)
    bs = L.as_f32(attention_score_bias, dev).reshape(1)
    cluster_h, pw, pws = AG.asap_attend(plan, x, sq, sh, bs, rate, 0 if seed is None else seed)   # :72-85

    node_score = le_conv(cluster_h, ei0, w0, le_conv_self_kernel, le_conv_self_bias, le_conv_aggr_self_kernel,
                         le_conv_aggr_self_bias, le_conv_aggr_neighbor_kernel, le_conv_aggr_neighbor_bias,
                         activation=None)                                                         # :87-91
    ngi = L.as_i32(node_graph_index, dev).reshape(-1)
    if prep.num_graphs is None:
        prep.num_graphs = int(ngi.max().item()) + 1 if n else 0
    idx = topk_pool(ngi, node_score, k=k, ratio=ratio, num_segments=prep.num_graphs)             # :93
    K = int(idx.shape[0])
    node_map = torch.full((n,), -1, dtype=torch.int32, device=dev)                               # :102-107
    node_map[idx.long()] = torch.arange(K, dtype=torch.int32, device=dev)
    topk_score = node_score if le_conv_activation is None else le_conv_activation(node_score)    # :94-96
    pooled_x = AG.gather_scale(cluster_h, idx, node_map, topk_score)                              # :98

    # S^T A1 S over (ei1, w1) = the edges without self-loops + the unit diagonal (:109-127)
    s_row_ptr, s_col, s_val = _assignment(plan, pw, pws, node_map)
    arn = torch.arange(n, dtype=torch.int32, device=dev)
    a_row = torch.cat([AG.plan_rows(plan).to(torch.int32), arn])
    a_col = torch.cat([plan.col, arn])
    a_val = None
    if w0 is not None:
        a_val = torch.cat([plan.edge_attr_to_csr(w0.detach()), torch.ones(n, dtype=torch.float32, device=dev)])
    row, col, val, row_ptr = sparse_sas(s_row_ptr, s_col, s_val, n, K, a_row, a_col, a_val, drop_diagonal=True)
    pooled_edge_index = _pooled_plan(row, col, row_ptr, K)
    pooled_edge_weight = torch.cat([val, torch.ones(K, dtype=torch.float32, device=dev)])
    pooled_ngi = gather_i32(ngi, idx)                                                             # :129
    if ei_np:
        pooled_edge_index = pooled_edge_index.cpu().numpy()
        pooled_edge_weight = pooled_edge_weight.cpu().numpy()
    if not isinstance(node_graph_index, torch.Tensor):
        pooled_ngi = pooled_ngi.cpu().numpy()
    return [pooled_x, pooled_edge_index, pooled_edge_weight, pooled_ngi]
