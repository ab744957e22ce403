# coding=utf-8
"""ASAP at a fixed shape (include/tfgx_asap_static.h): a StaticBatchGraph in, a StaticBatchGraph out, at capacities the host
computes (StaticBatchGraph.asap_pooled_capacities).  No host read, no sort: a hierarchical classifier with ASAP pooling over
GraphStore.collate_static batches can be captured in a hipGraph and replayed.

Reference: tf_geometric/nn/pool/asap.py:19-131 — the live part of the result is what nn.asap gives on collate(live ids in slot
order) with the slot number as the graph index; only the shapes are fixed and the padding is inert.

Self-loops.  nn.asap strips the self-loops of its input through a host read.  A static batch HAS self-loops — the padded unit
loops on its sinks, one live unit loop per cluster after an ASAP level — and its edge list is never compacted here.  Instead every
edge with row == col is ABSENT: the attention GCN and LEConv take its weight as 0 (one torch.where on the [e_cap] weights), the
attention kernel and the assignment kernel skip it, and A1 of S^T A1 S is the zero-masked weights plus the unit diagonal.  The
attention GCN gets a cache dict of its own (the plan only): batch.cache may hold the normalised adjacency another layer derived
from the unmasked weights under a key that does not see the weights.

A graph pooled to m_g clusters has at most m_g^2 edges whatever it had before, so the capacities do not compound:
max_nodes = m_max, max_edges = K_blk m_max with K_blk the most clusters of one graph (host arithmetic); they shrink from one ASAP
level to the next, though the first level's bound can exceed a sparse parent's max_edges.

Launches of the level's own device code, counted from this file and tfgx_asap_static.hip: attention 1, selection 2
(tfgx_static_pool_table, _select), pooled features 1, assignment 2 (zero S, scatter), A1 S 1, S^T (A1 S) 2 (tfgx_segment_gram_f32),
pooled edges and plans 3 (count, scan, emit) — 12, besides the GCN, the two aggregations and the small GEMMs that
nn.asap launches as well, and a handful of elementwise torch operators."""
import ctypes

import torch

from ... import _lib as L
from ... import autograd as AG
from ...data.graph import StaticBatchGraph
from ...plan import CsrPlan, CACHE_KEY_PLAN, attach_plan, attached_plan, segment_reduce
from ...sparse import SparseMatrix
from ..conv.gat import new_drop_seed
from ..conv.gcn import gcn
from ..conv.propagation import le_conv, _dense
from .dense_pool_static import _BlockEntries
from .sag_pool_static import _static_batch, attach_static_plans, select_static

CACHE_KEY_ASAP_STATIC = "tfgx_asap_static"


def _capacities(batch, capacities, k, ratio, what):
    made = batch.asap_pooled_capacities(k=k, ratio=ratio)            # validates k / ratio
    if capacities is not None and tuple(capacities) != tuple(made):
        raise ValueError("{}: capacities {} are not batch.asap_pooled_capacities(k={}, ratio={}) = {} (capacities below the bound "
                         "are not supported)".format(what, tuple(capacities), k, ratio, tuple(made)))
    return made


def asap_layout(P, pooled_row_ptr, counts, K, cap):
    """The launches of tfgx_asapstatic_edges on the blocks P [B K, K] (contiguous, not tracked; None when K == 0) at the pooled
    capacities `cap`; counts[2] is written in place: (edge_index, edge_src, edge_graph_index, [plan by row, plan by column] —
    still unlinked)."""
    lib = L.require_gpu()
    dev, B = pooled_row_ptr.device, cap.batch_size
    i32 = dict(dtype=torch.int32, device=dev)
    e_cap = cap.e_cap
    ei = torch.empty((2, e_cap), **i32)
    edge_src, egi = torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
    plans, ios = [], []
    for _ in range(2):
        row_ptr, col, perm = torch.empty(cap.n_cap + 1, **i32), torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
        io = L.CollatePlan()
        io.out_row_ptr, io.out_col, io.out_perm = row_ptr.data_ptr(), col.data_ptr(), perm.data_ptr()
        ios.append(io)
        plans.append(CsrPlan(row_ptr, col, perm, cap.n_cap, cap.n_cap, e_cap))
    ws_bytes = lib.tfgx_asapstatic_edges_workspace_bytes(B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a = L.AsapStaticEdgesArgs()
    a.P, a.ldp, a.pooled_row_ptr = (None if P is None else P.data_ptr()), K, pooled_row_ptr.data_ptr()
    a.B, a.K = B, K
    a.n_cap_out, a.e_cap, a.sinks, a.sink_degree = cap.n_cap, e_cap, cap.sinks, cap.sink_degree
    a.out_row, a.out_col, a.out_edge_src = ei.data_ptr(), ei.data_ptr() + 4 * e_cap, edge_src.data_ptr()
    a.out_edge_graph_index = egi.data_ptr()
    a.plan, a.plan_t = ctypes.pointer(ios[0]), ctypes.pointer(ios[1])
    a.counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.tfgx_asapstatic_edges(ctypes.byref(a), L.stream_ptr()), "tfgx_asapstatic_edges")
    return ei, edge_src, egi, plans


def asap_assignment(plan, pw, pws, sel, B, K, skip_self_loops=True):
    """S [n_cap, K] of tfgx_asapstatic_assign_f32: column c of the rows of slot g holds the attention weights of the slot's
    rank-c cluster (pw [e_cap] in the plan's CSR order, pws [n_cap] the self edges)."""
    lib = L.require_gpu()
    n = plan.n_dst
    S = torch.empty((n, K), dtype=torch.float32, device=pw.device)
    m_rows = sel.capacities.max_nodes
    L.check(lib.tfgx_asapstatic_assign_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), n, plan.num_edges, L.ptr(pw), L.ptr(pws),
                                           int(bool(skip_self_loops)), L.ptr(sel.node_index), L.ptr(sel.node_graph_index),
                                           L.ptr(sel.pooled_row_ptr), B, m_rows, K, L.ptr(S), K, L.stream_ptr()),
            "tfgx_asapstatic_assign_f32")
    return S


def asap_static(x, batch,
                attention_gcn_kernel, attention_gcn_bias,
                attention_query_kernel, attention_query_bias,
                attention_score_kernel, attention_score_bias,
                le_conv_self_kernel, le_conv_self_bias,
                le_conv_aggr_self_kernel, le_conv_aggr_self_bias,
                le_conv_aggr_neighbor_kernel,
                k=None, ratio=None, le_conv_activation=torch.sigmoid, drop_rate=0.0, training=None, seed=None, capacities=None):
    """
    ASAP on a static batch: the pooled StaticBatchGraph.

    :param x: [n_cap, num_features] node features of `batch` (differentiable; the rows of the dead nodes do not matter: they
        are replaced by zeros before anything reads them)
    :param batch: a StaticBatchGraph — GraphStore.collate_static's, or the result of a static pool.  Its edges with
        row == col are treated as absent (module docstring); a batch.edge_weight that requires grad is refused
    :param attention_* / le_conv_*: the eleven weights of nn.asap, in its order
    :param k / ratio: keep the top k (or num_nodes * ratio) clusters of every graph, ranked as nn.topk_pool ranks them
    :param drop_rate / training / seed: dropout on the attention weights by tfgx_dropout_keep(seed, position, drop_rate),
        position = the CSR position of the edge in the batch's plan, e_cap + i for the self edge of row i.  seed None: a fresh
        host integer when eager, a device seed (nn.conv.gat.new_drop_seed) while the stream is being captured, so that every
        replay draws new masks
    :param capacities: batch.asap_pooled_capacities(k, ratio) when None (nothing else is accepted)
    :return: the pooled batch.  x = (cluster_h * act(score))[node_index], differentiable wrt x and the eleven weights, dead
        rows exactly 0; the live edges are, slot by slot and row by row, the off-diagonal entries != 0.0 of S_g^T A1 S_g in
        column order and then the row's unit self-loop — the order in which nn.asap's CSR plan walks a row; edge_weight is
        detached (1.0 on self-loops and padding); edge_src maps a pooled edge to its entry of P (-1: self-loop or padding),
        node_index a pooled row to its parent row (-1: dead), node_score holds the raw cluster scores [n_cap] the selection
        ranked, asap_blocks the blocks P [B K_blk, K_blk] (None when K_blk == 0).  y, ids and graph_mask are the parent's; all three plans are attached and cached as collate_static does it.

    No host read and no sort.  More than TFGX_SEGGRAM_MAX_K clusters of one graph (K_blk, host arithmetic) are refused.
    """
    what = "asap_static"
    store = _static_batch(batch, what)
    parent = batch.capacities
    B, n_cap, e_cap = parent.batch_size, parent.n_cap, parent.e_cap
    if batch.edge_weight is not None and AG.needs_grad(batch.edge_weight):
        raise ValueError("{}: edge_weight requires grad; the static route does not differentiate edge weights (detach it, or use "
                         "nn.asap)".format(what))
    if not hasattr(x, "shape") or len(x.shape) != 2 or int(x.shape[0]) != n_cap:
        raise ValueError("{}: x must have one row per row of the batch ([{}, F]), got shape {}".format(
            what, n_cap, tuple(getattr(x, "shape", ()))))
    if int(batch.node_graph_index.shape[0]) != n_cap or int(batch.edge_index.shape[-1]) != e_cap or \
            int(batch.graph_row_ptr.shape[0]) != B + 2:
        raise ValueError("{}: capacities {} do not describe the batch ({} rows, {} edges, {} slots)".format(
            what, tuple(parent), int(batch.node_graph_index.shape[0]), int(batch.edge_index.shape[-1]),
            int(batch.graph_row_ptr.shape[0]) - 2))
    cap = _capacities(batch, capacities, k, ratio, what)
    K = batch.asap_clusters_per_graph(k=k, ratio=ratio)
    if K > L.SEGGRAM_MAX_K:
        raise ValueError("{}: K_blk = {} clusters of one graph (k / ratio applied to the batch's largest graph of {} nodes) is "
                         "more than TFGX_SEGGRAM_MAX_K = {}".format(what, K, batch.max_graph_nodes(), L.SEGGRAM_MAX_K))
    plan = batch.cache.get(CACHE_KEY_PLAN) or attached_plan(batch.edge_index)
    if plan is None or plan._transposed is None:
        raise ValueError("{}: the batch has lost the plans collate_static attached (edge_index written in place, or its cache "
                         "cleared)".format(what))
    L.require_gpu()
    dev = batch.edge_index.device
    d = store._resident()
    arange = store._identity(d, max(cap.n_cap, n_cap) + 1)      # refuses to grow inside a capture, by name
    f32 = dict(dtype=torch.float32, device=dev)
    zero = torch.zeros((), **f32)

    # dead rows exactly 0 before anything reads them: garbage there (a NaN times a zero gradient) must not reach a weight gradient
    x = torch.where((batch.node_graph_index < B)[:, None], L.as_f32(x, dev), zero)
    ei = batch.edge_index
    gnn_ei = ei if attached_plan(ei) is not None else attach_plan(ei.view(ei.shape), plan)
    w = torch.ones(e_cap, **f32) if batch.edge_weight is None else L.as_f32(batch.edge_weight, dev).detach().reshape(-1)
    if int(w.shape[0]) != e_cap:
        raise ValueError("{}: edge_weight has {} entries, the batch has {} edges".format(what, int(w.shape[0]), e_cap))
    w0 = torch.where(ei[0] == ei[1], zero, w)                   # an edge row == col is absent
    rate = float(drop_rate) if (training and drop_rate > 0) else 0.0
    if rate > 0.0 and seed is None:
        seed = new_drop_seed(dev)

    gcn_cache = batch.cache.setdefault(CACHE_KEY_ASAP_STATIC, {CACHE_KEY_PLAN: plan})
    h = gcn(x, SparseMatrix(gnn_ei, w0, [n_cap, n_cap]), attention_gcn_kernel, attention_gcn_bias, cache=gcn_cache)   # asap.py:54
    hmax = AG.aggregate(plan, h, L.MAX) if AG.needs_grad(h) else segment_reduce(plan, h, L.MAX)
    query = _dense(torch.maximum(hmax, h), attention_query_kernel, attention_query_bias)          # :57-65
    A = int(h.shape[1])
    ks = L.as_f32(attention_score_kernel, dev)
    if tuple(ks.shape) != (2 * A, 1):
        raise ValueError("{}: attention_score_kernel must be [{}, 1], got {}".format(what, 2 * A, tuple(ks.shape)))
    sq = _dense(query, ks[:A]).reshape(-1)
    sh = _dense(h, ks[A:]).reshape(-1)
    bs = L.as_f32(attention_score_bias, dev).reshape(1)
    cluster_h, pw, pws = AG.asap_attend(plan, x, sq, sh, bs, rate, 0 if seed is None else seed, skip_self_loops=True)   # :72-85

    node_score = le_conv(cluster_h, gnn_ei, w0, le_conv_self_kernel, le_conv_self_bias, le_conv_aggr_self_kernel,
                         le_conv_aggr_self_bias, le_conv_aggr_neighbor_kernel, None, activation=None)     # :87-91
    sel = select_static(batch, node_score, k, ratio, cap, what)                                           # :93
    topk_score = node_score if le_conv_activation is None else le_conv_activation(node_score)             # :94-96
    px = AG.gather_scale_static(cluster_h, sel.node_index, sel.node_map, topk_score)                      # :98

    # P_g = S_g^T (A1 S)_g over the B slot segments, A1 = the zero-masked weights + the unit diagonal (:109-127)
    P = None
    if K > 0:
        S = asap_assignment(plan, pw.detach(), pws.detach(), sel, B, K)
        A1S = segment_reduce(plan, S, L.SUM, w_csr=plan.edge_attr_to_csr(w0), self_coef=torch.ones(n_cap, **f32))
        nodes = arange[:n_cap]
        graph_plan = CsrPlan(batch.graph_row_ptr[:B + 1], nodes, nodes, B, n_cap, n_cap)
        P = AG.segment_gram_forward(graph_plan, S, A1S)                                                  # [B K, K]
    pei, edge_src, egi, plans = asap_layout(P, sel.pooled_row_ptr, sel.counts, K, cap)
    pooled_w = _BlockEntries.apply(P.reshape(-1) if P is not None else torch.zeros(0, **f32), edge_src)

    pooled = StaticBatchGraph(px, pei, sel.node_graph_index, egi, batch.y, pooled_w, batch.ids, batch.graph_mask, sel.counts, cap,
                              batch._store_len, given_ids=batch._given_ids)
    pooled._store, pooled.graph_row_ptr = store, sel.pooled_row_ptr
    pooled.node_index, pooled.edge_src = sel.node_index, edge_src
    pooled.node_score, pooled.asap_blocks = node_score.detach().reshape(-1), P
    pooled._degree_bound = pooled._node_bound = K               # a pooled graph has at most K rows, a pooled row at most K edges
    attach_static_plans(pooled, store, plans, arange, K)
    return pooled
