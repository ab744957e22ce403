# coding=utf-8
"""SAGPool at a fixed shape (include/tfgx_pool_static.h): a StaticBatchGraph in, a StaticBatchGraph out, at capacities the host
computes (StaticBatchGraph.pooled_capacities).  No host read, no sort: the level is a fixed sequence of seven launches, so a
hierarchical classifier over GraphStore.collate_static batches can be captured in a hipGraph and replayed.

Reference: tf_geometric/nn/pool/sag_pool.py:7-45 and nn/pool/topk_pool.py:6-87 — the same selection (score descending, ties in
input order) and the same induced subgraph as nn.sag_pool; only the shapes are fixed and the padding is inert."""
import ctypes

import torch

from ... import _lib as L
from ...data.graph import StaticBatchGraph
from ...plan import CsrPlan, CACHE_KEY_PLAN, attach_plan, attached_plan, hub_policy
from .common_pool import CACHE_KEY_GRAPH_PLAN


class StaticTopK(object):
    """What topk_pool_static returns, all on the device: node_index int32 [n_cap'] (pooled row -> parent row, slot by slot in
    rank order, -1 for a dead row), node_map int32 [n_cap] (parent row -> pooled row or -1), pooled_row_ptr int32 [B + 2] (the
    slots' pooled offsets, then the live total, closed with n_cap'), node_graph_index int32 [n_cap'] (slot, or B), counts int32
    [4] (live graphs, live pooled nodes, 0 until the edges are pooled, flags) and the pooled `capacities`."""

    def __init__(self, node_index, node_map, pooled_row_ptr, node_graph_index, counts, capacities):
        self.node_index = node_index
        self.node_map = node_map
        self.pooled_row_ptr = pooled_row_ptr
        self.node_graph_index = node_graph_index
        self.counts = counts
        self.capacities = capacities


def _static_batch(batch, what):
    if not isinstance(batch, StaticBatchGraph):
        raise ValueError("{}: batch must be a StaticBatchGraph (GraphStore.collate_static, or a pooled one), got {}".format(
            what, type(batch).__name__))
    store = batch._store
    if store is None or batch.graph_row_ptr is None:
        raise ValueError("{}: the batch does not come from GraphStore.collate_static (no store, no graph_row_ptr)".format(what))
    largest = store._max_graph_nodes()
    if largest > L.STATIC_POOL_MAX_GRAPH_NODES:
        raise ValueError("{}: the store's largest graph has {} nodes, more than the {} the static pooling route ranks in LDS "
                         "(TFGX_STATIC_POOL_MAX_GRAPH_NODES): use nn.sag_pool on collate batches".format(
                             what, largest, L.STATIC_POOL_MAX_GRAPH_NODES))
    return store


def _pooled_capacities(batch, capacities, k, ratio, what):
    made = batch.pooled_capacities(k=k, ratio=ratio)            # validates k / ratio
    if capacities is None:
        return made
    parent = batch.capacities
    if capacities.batch_size != parent.batch_size:
        raise ValueError("{}: capacities for {} slots, the batch has {}".format(what, capacities.batch_size, parent.batch_size))
    same = ("max_edges", "sink_degree", "sinks", "e_cap")
    if any(getattr(capacities, f) != getattr(parent, f) for f in same) or capacities.max_nodes > parent.max_nodes or \
            capacities.n_cap != capacities.max_nodes + capacities.sinks:
        raise ValueError("{}: capacities {} were made for other parent capacities than the batch's {} (a pooled level keeps "
                         "max_edges, sink_degree and sinks, and does not grow max_nodes)".format(what, tuple(capacities),
                                                                                                  tuple(parent)))
    return capacities


def topk_pool_static(batch, score, k=None, ratio=None, capacities=None):
    """The nodes nn.topk_pool(node_graph_index, score, k / ratio) keeps of every slot of a static batch, at a fixed shape:
    a StaticTopK.  Two launches (tfgx_static_pool_table, tfgx_static_pool_select: one workgroup per slot ranks the slot's
    nodes in LDS), no host read.  `score` holds one value per row of the batch ([n_cap] or [n_cap, 1]); what the dead rows
    hold does not matter.  `capacities`: batch.pooled_capacities(k, ratio) when None."""
    what = "topk_pool_static"
    _static_batch(batch, what)
    return select_static(batch, score, k, ratio, _pooled_capacities(batch, capacities, k, ratio, what), what)


def select_static(batch, score, k, ratio, cap, what):
    """The two launches of the selection at the pooled capacities `cap` (max_nodes, n_cap and sinks are read; nn.asap_static
    brings capacities whose edges and sinks are not the parent's): a StaticTopK.  tfgx_static_pool_select takes ONE sink count
    and uses it only to hold the live totals to n_cap - sinks and n_cap' - sinks: the smaller of the two counts keeps both
    bounds inside the arrays and at or above max_nodes (a SAG level has the parent's sinks: nothing changes for it)."""
    lib = L.require_gpu()
    parent = batch.capacities
    B, n_cap = parent.batch_size, parent.n_cap
    dev = batch.edge_index.device
    sc = L.as_f32(score, dev).detach()
    if sc.numel() != n_cap:
        raise ValueError("{}: score must hold one value per row of the batch ({}), got shape {}".format(what, n_cap,
                                                                                                          tuple(sc.shape)))
    sc = sc.reshape(-1).contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    pooled_row_ptr, counts = torch.empty(B + 2, **i32), torch.empty(4, **i32)
    node_index, ngi, node_map = torch.empty(cap.n_cap, **i32), torch.empty(cap.n_cap, **i32), torch.empty(n_cap, **i32)
    stream = L.stream_ptr()
    L.check(lib.tfgx_static_pool_table(L.ptr(batch.graph_row_ptr), L.ptr(batch.counts), B, -1 if k is None else int(k),
                                       0.0 if ratio is None else float(ratio), cap.max_nodes, cap.n_cap, L.ptr(pooled_row_ptr),
                                       L.ptr(counts), stream), "tfgx_static_pool_table")
    L.check(lib.tfgx_static_pool_select(L.ptr(sc), L.ptr(batch.graph_row_ptr), L.ptr(pooled_row_ptr), B, n_cap,
                                        min(parent.sinks, cap.sinks), cap.n_cap, L.ptr(node_index), L.ptr(ngi), L.ptr(node_map), stream),
            "tfgx_static_pool_select")
    return StaticTopK(node_index, node_map, pooled_row_ptr, ngi, counts, cap)


def sag_pool_static(x, batch, score_gnn, k=None, ratio=None, score_activation=None, training=None, capacities=None):
    """
    SAGPool on a static batch: the pooled StaticBatchGraph.

    :param x: [n_cap, num_features] node features of `batch` (differentiable; the rows of the dead nodes do not matter)
    :param batch: a StaticBatchGraph — GraphStore.collate_static's, or the result of an earlier sag_pool_static
    :param score_gnn: [x, edge_index, edge_weight] => node_score ([n_cap, 1]); called with cache=batch.cache
    :param k / ratio: keep top k (or num_nodes * ratio) nodes of every graph, by the rule of nn.topk_pool
    :param score_activation: applied to node_score AFTER the ranking, before it multiplies the features
    :param capacities: batch.pooled_capacities(k, ratio) when None
    :return: the pooled batch.  Its x is (x * act(score))[node_index], differentiable wrt x and the score, with dead rows
        exactly 0; it carries edge_index / edge_weight / node_graph_index / edge_graph_index at the pooled capacities, y, ids and
        graph_mask shared with the parent, its own counts and capacities, node_index and edge_id, and all three plans attached
        and cached the way collate_static does it.  readout, check, pooled_capacities, GCN layers with cache=pooled.cache and a
        further sag_pool_static work on it as on the parent.
    """
    from ... import autograd as AG
    what = "sag_pool_static"
    store = _static_batch(batch, what)
    parent = batch.capacities
    B, n_cap, e_cap = parent.batch_size, parent.n_cap, parent.e_cap
    if batch.edge_weight is not None and AG.needs_grad(batch.edge_weight):
        raise ValueError("{}: edge_weight requires grad; the static route does not differentiate edge weights (use "
                         "nn.sag_pool)".format(what))
    if not hasattr(x, "shape") or len(x.shape) != 2 or int(x.shape[0]) != n_cap:
        raise ValueError("{}: x must have one row per row of the batch ([{}, F]), got shape {}".format(
            what, n_cap, tuple(getattr(x, "shape", ()))))
    cap = _pooled_capacities(batch, capacities, k, ratio, what)
    plan = batch.cache.get(CACHE_KEY_PLAN) or attached_plan(batch.edge_index)
    if plan is None or plan._transposed is None:
        raise ValueError("{}: the batch has lost the plans collate_static attached (edge_index written in place, or its cache "
                         "cleared)".format(what))
    plan_t = plan._transposed
    lib = L.require_gpu()
    d = store._resident()
    arange = store._identity(d, cap.n_cap + 1)                  # refuses to grow inside a capture, by name

    gnn_edge_index = batch.edge_index
    if attached_plan(gnn_edge_index) is None:                   # an alias carrying the parent plan: the caller's tensor is left alone
        gnn_edge_index = attach_plan(batch.edge_index.view(batch.edge_index.shape), plan)
    node_score = score_gnn([x, gnn_edge_index, batch.edge_weight], training=training, cache=batch.cache)
    sel = topk_pool_static(batch, node_score, k=k, ratio=ratio, capacities=cap)
    if score_activation is not None:
        node_score = score_activation(node_score)

    dev = batch.edge_index.device
    i32 = dict(dtype=torch.int32, device=dev)
    ei = torch.empty((2, e_cap), **i32)
    edge_id, egi = torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
    w = torch.empty(e_cap, dtype=torch.float32, device=dev)
    plans, ios = [], []
    for pp in (plan, plan_t):
        row_ptr, col, perm = torch.empty(cap.n_cap + 1, **i32), torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
        io = L.CollatePlan()
        io.ds_row_ptr, io.ds_col, io.ds_perm = pp.row_ptr.data_ptr(), pp.col.data_ptr(), pp.perm.data_ptr()
        io.out_row_ptr, io.out_col, io.out_perm = row_ptr.data_ptr(), col.data_ptr(), perm.data_ptr()
        ios.append(io)
        plans.append(CsrPlan(row_ptr, col, perm, cap.n_cap, cap.n_cap, e_cap))
    ws_bytes = lib.tfgx_static_pool_edges_workspace_bytes(cap.n_cap, e_cap)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pw = None if batch.edge_weight is None else L.as_f32(batch.edge_weight, dev).detach().reshape(-1).contiguous()
    pei = batch.edge_index
    a = L.StaticPoolArgs()
    a.row, a.col = pei.data_ptr(), pei.data_ptr() + 4 * e_cap
    a.w = None if pw is None else pw.data_ptr()
    a.edge_graph_index = batch.edge_graph_index.data_ptr()
    a.n_cap, a.e_cap, a.B, a.sinks, a.sink_degree = n_cap, e_cap, B, parent.sinks, parent.sink_degree
    a.node_map, a.node_index, a.pooled_row_ptr = sel.node_map.data_ptr(), sel.node_index.data_ptr(), sel.pooled_row_ptr.data_ptr()
    a.n_cap_out = cap.n_cap
    a.out_row, a.out_col, a.out_edge_id = ei.data_ptr(), ei.data_ptr() + 4 * e_cap, edge_id.data_ptr()
    a.out_edge_graph_index, a.out_w = egi.data_ptr(), w.data_ptr()
    a.plan, a.plan_t = ctypes.pointer(ios[0]), ctypes.pointer(ios[1])
    a.counts, a.workspace, a.workspace_bytes = sel.counts.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.tfgx_static_pool_edges(ctypes.byref(a), L.stream_ptr()), "tfgx_static_pool_edges")

    px = AG.gather_scale_static(L.as_f32(x, dev), sel.node_index, sel.node_map, node_score)

    pooled = StaticBatchGraph(px, ei, sel.node_graph_index, egi, batch.y, w, batch.ids, batch.graph_mask, sel.counts, cap,
                              batch._store_len, given_ids=batch._given_ids)
    pooled._store, pooled.graph_row_ptr = store, sel.pooled_row_ptr
    pooled.node_index, pooled.edge_id = sel.node_index, edge_id
    pooled._degree_bound, pooled._node_bound = batch._degree_bound, batch._node_bound
    # no pooled row is longer than its parent row, and a sink holds sink_degree edges as before: the rule of collate_static
    attach_static_plans(pooled, store, plans, arange, batch.max_degree())
    return pooled


def attach_static_plans(pooled, store, plans, arange, max_degree):
    """Link the two edge plans a static pool derived for `pooled`, and the graph plan over its graph_row_ptr, and attach and
    cache all three the way collate_static does.  `max_degree` bounds the edges of a live row of either edge plan; with the
    sink degree it decides, by plan.hub_policy's threshold for these capacities, whether both are marked as having no hub rows
    and no walk order.  `arange`: the store's identity array, at least n_cap + 1 long."""
    cap, ei, ngi = pooled.capacities, pooled.edge_index, pooled.node_graph_index
    B = cap.batch_size
    new_plan, new_plan_t = plans
    new_plan._edge_index = ei
    new_plan._transposed, new_plan_t._transposed = new_plan_t, new_plan
    thr, _ = hub_policy(cap.e_cap, cap.n_cap)
    if max(max_degree, cap.sink_degree) <= thr:
        for pl in plans:
            pl.hub_threshold, pl._hub, pl._row_order = thr, False, False
    attach_plan(ei, new_plan)
    pooled.cache[CACHE_KEY_PLAN] = new_plan
    nodes = arange[:cap.n_cap]
    graph_plan = CsrPlan(pooled.graph_row_ptr, nodes, nodes, B + 1, cap.n_cap, cap.n_cap)
    graph_plan._transposed = CsrPlan(arange[:cap.n_cap + 1], ngi, nodes, cap.n_cap, B + 1, cap.n_cap)
    graph_plan._transposed._transposed = graph_plan
    for pl, rows in ((graph_plan, B + 1), (graph_plan._transposed, cap.n_cap)):
        pl.hub_threshold, pl._hub, pl._row_order = hub_policy(cap.n_cap, rows)[0], False, False
    pooled.cache[CACHE_KEY_GRAPH_PLAN] = (ngi, ngi._version, graph_plan)
