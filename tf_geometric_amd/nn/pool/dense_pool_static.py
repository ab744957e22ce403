# coding=utf-8
"""DiffPool and MinCutPool at a fixed shape (include/tfgx_dense_pool_static.h): a StaticBatchGraph in, a StaticBatchGraph out,
at capacities the host computes (StaticBatchGraph.dense_pooled_capacities).  No host read, no sort: a hierarchical classifier
with dense pooling over GraphStore.collate_static batches can be captured in a hipGraph and replayed.

Reference: tf_geometric/nn/pool/diff_pool.py:8-105 and nn/pool/min_cut_pool.py:18-232 — the same coarsening and the same
losses as nn.diff_pool / nn.min_cut_pool on collate(live ids in slot order), with the slot number as the graph index; only the
shapes are fixed and the padding is inert.

Every live slot becomes exactly K pooled rows and at most K K pooled edges, so the pooled capacities are B K rows and B K K
edges whatever the batch holds, and they do not compound over levels.  A S runs on the plan the batch carries; P = S_g^T (A S)_g,
the pooled features and the K x K blocks of the MinCut losses are the segmented product (include/tfgx_seggram.h) over the B
slot segments — the dead graph B is never a segment, so its long row is never walked; the pooled edge list, both plans and the
node tables are three launches of tfgx_dense_pool_static.  An edge between two graphs cannot occur in a batch made by
collate_static or by a static pool (every edge is copied or derived inside its slot's row range), so, unlike nn.diff_pool, no
verdict on cross-graph edges is computed or read."""
import ctypes

import numpy as np
import torch

from ... import _lib as L
from ... import autograd as AG
from ...data.graph import StaticBatchGraph
from ...plan import CsrPlan, attach_plan, attached_plan, CACHE_KEY_PLAN
from ..conv.propagation import _refuse_trainable_edge_weight
from .diff_pool import _adjacency_times, _check_assign
from .sag_pool_static import _static_batch, attach_static_plans


class _Carried(object):
    """What the static dense pools need of a batch: the edge plan it carries, the graph plan over its B slot segments, the
    sizes."""

    def __init__(self, what, batch):
        self.store = _static_batch(batch, what)
        cap = batch.capacities
        self.B, self.n_cap, self.e_cap = cap.batch_size, cap.n_cap, cap.e_cap
        if int(batch.node_graph_index.shape[0]) != self.n_cap or int(batch.edge_index.shape[-1]) != self.e_cap or \
                int(batch.graph_row_ptr.shape[0]) != self.B + 2 or cap.n_cap != cap.max_nodes + cap.sinks:
            raise ValueError("{}: capacities {} do not describe the batch ({} rows, {} edges, {} slots)".format(
                what, tuple(cap), int(batch.node_graph_index.shape[0]), int(batch.edge_index.shape[-1]),
                int(batch.graph_row_ptr.shape[0]) - 2))
        plan = batch.cache.get(CACHE_KEY_PLAN) or attached_plan(batch.edge_index)
        if plan is None or plan._transposed is None:
            raise ValueError("{}: the batch has lost the plans collate_static attached (edge_index written in place, or its cache "
                             "cleared)".format(what))
        self.plan = plan
        self.batch = batch
        self.dev = batch.edge_index.device
        nodes = self.store._identity(self.store._resident(), self.n_cap)
        self.ids = batch.node_graph_index                           # B on dead rows: zero rows in the product's backward
        self.graph_plan = CsrPlan(batch.graph_row_ptr[:self.B + 1], nodes, nodes, self.B, self.n_cap, self.n_cap)

    def rows(self, what, name, t):
        t = L.as_f32(t, self.dev)
        if t.dim() != 2 or int(t.shape[0]) != self.n_cap:
            raise ValueError("{}: {} must have one row per row of the batch ([{}, F]), got shape {}".format(
                what, name, self.n_cap, tuple(t.shape)))
        return t

    def gram(self, S, Y):
        return AG.segment_gram(self.graph_plan, self.ids, S, Y)

    def gnn_edge_index(self):
        """The batch's edge_index, or an alias carrying the plan when the caller's tensor has lost it (left alone)."""
        ei = self.batch.edge_index
        if attached_plan(ei) is None:
            ei = attach_plan(ei.view(ei.shape), self.plan)
        return ei


class _BlockEntries(torch.autograd.Function):
    """where(edge_src >= 0, P.flat[edge_src], 1.0): the weights of the pooled edges.  The live entries of edge_src are distinct,
    so the backward is a plain scatter into zeros (the padded edges land on one spare entry that is cut off): no sort, no
    accumulation, nothing that depends on an order."""

    @staticmethod
    def forward(ctx, flat, edge_src):
        n = int(flat.shape[0])
        ctx.n = n
        ctx.save_for_backward(edge_src)
        if n == 0:
            return torch.ones(int(edge_src.shape[0]), dtype=torch.float32, device=flat.device)
        return torch.where(edge_src >= 0, flat[edge_src.clamp(min=0).long()], torch.ones((), dtype=torch.float32, device=flat.device))

    @staticmethod
    def backward(ctx, g):
        (edge_src,) = ctx.saved_tensors
        at = torch.where(edge_src >= 0, edge_src, torch.full((), ctx.n, dtype=edge_src.dtype, device=edge_src.device)).long()
        d = torch.zeros(ctx.n + 1, dtype=torch.float32, device=g.device)
        d.scatter_(0, at, g.to(torch.float32))
        return d[:ctx.n], None


def _assign(what, car, dense_assign, num_clusters=None):
    if not hasattr(dense_assign, "shape") or len(dense_assign.shape) != 2 or int(dense_assign.shape[0]) != car.n_cap:
        raise ValueError("{}: dense_assign must have one row per row of the batch ([{}, K]), got shape {}".format(
            what, car.n_cap, tuple(getattr(dense_assign, "shape", ()))))
    S, _, K = _check_assign(what, L.as_f32(dense_assign, car.dev), None, num_clusters)
    return S, K


def _normed_weight(what, car, edge_weight):
    """utils.adj_norm_edge(add_self_loop=False) on the carried plan: D^-1/2 A D^-1/2 with D the row sums, no plan is built.
    The padded self-loops live on the sinks (degree d, weight 1 / d): inert."""
    _refuse_trainable_edge_weight(edge_weight, what)
    lib = L.require_gpu()
    ei = car.batch.edge_index
    w = torch.ones(car.e_cap, dtype=torch.float32, device=car.dev) if edge_weight is None else \
        L.as_f32(edge_weight, car.dev).detach().reshape(-1)
    if int(w.shape[0]) != car.e_cap:
        raise ValueError("{}: edge_weight has {} entries, the batch has {} edges".format(what, int(w.shape[0]), car.e_cap))
    deg = torch.empty(car.n_cap, dtype=torch.float32, device=car.dev)
    L.check(lib.tfgx_segment_weight_sum_f32(L.ptr(car.plan.row_ptr), L.ptr(car.plan.edge_attr_to_csr(w)), car.n_cap, 0.0,
                                            L.ptr(deg), L.stream_ptr()), "tfgx_segment_weight_sum_f32")
    dis = torch.pow(deg, -0.5)
    dis = torch.where(torch.isinf(dis) | torch.isnan(dis), torch.zeros_like(dis), dis)
    return dis[ei[0].long()] * w * dis[ei[1].long()]


def dense_pool_layout(P, batch, K, drop_diagonal, cap):
    """The three launches of tfgx_dense_pool_static on the blocks P [B K, K] (contiguous, not tracked) of `batch`, at the pooled
    capacities `cap`: (pooled_row_ptr, counts, node_index, node_graph_index, node_map, edge_index, edge_src, edge_graph_index,
    [plan by row, plan by column] — still unlinked)."""
    lib = L.require_gpu()
    dev, B = P.device, cap.batch_size
    i32 = dict(dtype=torch.int32, device=dev)
    e_cap = cap.e_cap
    pooled_row_ptr, counts = torch.empty(B + 2, **i32), torch.empty(4, **i32)
    node_index, ngi, node_map = torch.empty(cap.n_cap, **i32), torch.empty(cap.n_cap, **i32), torch.empty(B * K, **i32)
    ei = torch.empty((2, e_cap), **i32)
    edge_src, egi = torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
    plans, ios = [], []
    for _ in range(2):
        row_ptr, col, perm = torch.empty(cap.n_cap + 1, **i32), torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
        io = L.CollatePlan()
        io.out_row_ptr, io.out_col, io.out_perm = row_ptr.data_ptr(), col.data_ptr(), perm.data_ptr()
        ios.append(io)
        plans.append(CsrPlan(row_ptr, col, perm, cap.n_cap, cap.n_cap, e_cap))
    ws_bytes = lib.tfgx_dense_pool_static_workspace_bytes(B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a = L.DensePoolStaticArgs()
    a.P, a.ldp, a.graph_mask, a.parent_counts = P.data_ptr(), K, batch.graph_mask.data_ptr(), batch.counts.data_ptr()
    a.B, a.K, a.drop_diagonal = B, K, int(bool(drop_diagonal))
    a.n_cap_out, a.e_cap, a.sinks, a.sink_degree = cap.n_cap, e_cap, cap.sinks, cap.sink_degree
    a.pooled_row_ptr, a.node_index, a.node_graph_index = pooled_row_ptr.data_ptr(), node_index.data_ptr(), ngi.data_ptr()
    a.node_map = node_map.data_ptr()
    a.out_row, a.out_col, a.out_edge_src = ei.data_ptr(), ei.data_ptr() + 4 * e_cap, edge_src.data_ptr()
    a.out_edge_graph_index = egi.data_ptr()
    a.plan, a.plan_t = ctypes.pointer(ios[0]), ctypes.pointer(ios[1])
    a.counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws_bytes
    L.check(lib.tfgx_dense_pool_static(ctypes.byref(a), L.stream_ptr()), "tfgx_dense_pool_static")
    return pooled_row_ptr, counts, node_index, ngi, node_map, ei, edge_src, egi, plans


def _coarsen_static(what, car, x, adjacency_weight, S, K, drop_diagonal, bias=None, activation=None):
    batch, dev = car.batch, car.dev
    cap = batch.dense_pooled_capacities(K, drop_diagonal=drop_diagonal)
    if x is not None:
        x = car.rows(what, "x", x)
    w = None
    if adjacency_weight is not None:
        w = L.as_f32(adjacency_weight, dev).reshape(-1)
        if int(w.shape[0]) != car.e_cap:
            raise ValueError("{}: edge_weight has {} entries, the batch has {} edges".format(what, int(w.shape[0]), car.e_cap))
    L.require_gpu()
    arange = car.store._identity(car.store._resident(), cap.n_cap + 1)     # refuses to grow inside a capture, by name
    P = car.gram(S, _adjacency_times(car, S, w))                            # [B K, K], cluster_pool.py:36
    slot_x = None if x is None else car.gram(S, x)                          # [B K, F], cluster_pool.py:42
    pooled_row_ptr, counts, node_index, ngi, node_map, ei, edge_src, egi, plans = dense_pool_layout(
        P.detach(), batch, K, drop_diagonal, cap)

    pw = _BlockEntries.apply(P.reshape(-1), edge_src)
    px = None
    if slot_x is not None:
        px = AG.gather_scale_static(slot_x, node_index, node_map)          # dead rows exactly 0
        if bias is not None or activation is not None:
            h = px if bias is None else AG.bias_add(px, L.as_f32(bias, dev))          # diff_pool.py:99-100
            if activation is not None:
                h = activation(h)
            px = torch.where((node_index >= 0)[:, None], h, torch.zeros((), dtype=torch.float32, device=dev))

    pooled = StaticBatchGraph(px, ei, ngi, egi, batch.y, pw, batch.ids, batch.graph_mask, counts, cap, batch._store_len,
                              given_ids=batch._given_ids)
    pooled._store, pooled.graph_row_ptr = car.store, pooled_row_ptr
    pooled.node_index, pooled.edge_src = node_index, edge_src
    pooled._degree_bound = K                                    # a pooled row holds at most K edges, whatever the dataset's degrees
    pooled._node_bound = K                                      # ... and a pooled graph exactly K nodes
    attach_static_plans(pooled, car.store, plans, arange, K)
    return pooled


def diff_pool_coarsen_static(x, batch, dense_assign):
    """
    diff_pool_coarsen on a static batch: the pooled StaticBatchGraph.

    :param x: [n_cap, F] node features of `batch` or None (differentiable; the rows of the dead nodes do not matter)
    :param batch: a StaticBatchGraph — GraphStore.collate_static's, or the result of a static pool
    :param dense_assign: [n_cap, K] assignment of every node to the K clusters of ITS graph, K <= TFGX_SEGGRAM_MAX_K
    :return: the pooled batch at batch.dense_pooled_capacities(K): every live slot owns K rows (x = S_g^T x_g, dead rows
        exactly 0) and the entries != 0.0 of S_g^T A_g S_g as edges, in row-major order, with edge_weight differentiable in
        dense_assign and in a tracked batch.edge_weight; edge_src maps a pooled edge to its entry of S^T A S (-1: padding),
        node_index a pooled row to slot * K + cluster (-1: dead).  y, ids and graph_mask are the parent's; all three plans are
        attached and cached as collate_static does it.

    No host read and no sort.  No edge of a static batch joins two graphs, so no verdict is read (module docstring).
    """
    what = "diff_pool_coarsen_static"
    car = _Carried(what, batch)
    S, K = _assign(what, car, dense_assign)
    return _coarsen_static(what, car, x, batch.edge_weight, S, K, False)


def diff_pool_static(x, batch, feature_gnn, assign_gnn, num_clusters, bias=None, activation=None, training=None):
    """
    DiffPool on a static batch (nn.diff_pool's arguments with `batch` for the four graph tensors): the pooled StaticBatchGraph.

    :param feature_gnn / assign_gnn: callables [x, edge_index, edge_weight] -> [n_cap, F'] / [n_cap, num_clusters]; called with
        training= and cache=batch.cache
    :param bias / activation: applied to the LIVE pooled rows; dead rows stay exactly 0
    """
    what = "diff_pool_static"
    car = _Carried(what, batch)
    x = car.rows(what, "x", x)
    edge_weight = batch.edge_weight
    if edge_weight is None:                                                # diff_pool.py:78-80
        edge_weight = torch.ones(car.e_cap, dtype=torch.float32, device=car.dev)
    inputs = [x, car.gnn_edge_index(), edge_weight]
    assign_logits = assign_gnn(inputs, training=training, cache=batch.cache)
    h = feature_gnn(inputs, training=training, cache=batch.cache)
    S, K = _assign(what, car, torch.softmax(L.as_f32(assign_logits), dim=-1), num_clusters)        # :92
    return _coarsen_static(what, car, h, edge_weight, S, K, False, bias=bias, activation=activation)


def min_cut_pool_coarsen_static(x, batch, dense_assign, normed_edge_weight=None):
    """min_cut_pool_coarsen on a static batch: diff_pool_coarsen_static on the normalised weights D^-1/2 A D^-1/2 (computed on
    the carried plan when normed_edge_weight is None; a batch.edge_weight that requires grad is then refused, as
    nn.min_cut_pool_coarsen refuses it), without the pooled self-loops."""
    what = "min_cut_pool_coarsen_static"
    car = _Carried(what, batch)
    S, K = _assign(what, car, dense_assign)
    if normed_edge_weight is None:
        normed_edge_weight = _normed_weight(what, car, batch.edge_weight)
    return _coarsen_static(what, car, x, normed_edge_weight, S, K, True)


def _losses_static(car, S, K, w):
    B, dev, mask = car.B, car.dev, car.batch.graph_mask
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    live = car.batch.counts[0].clamp(min=1).to(torch.float32)
    degree = _adjacency_times(car, torch.ones((car.n_cap, 1), dtype=torch.float32, device=dev), w)        # min_cut_pool.py:29
    blocks = lambda Y: car.gram(S, Y).reshape(B, K, K)                                                    # noqa: E731
    trace = lambda M: torch.diagonal(M, dim1=1, dim2=2).sum(dim=-1)                                       # noqa: E731
    intra_edge_sum = trace(blocks(_adjacency_times(car, S, w)))                                           # :64
    all_edge_sum = trace(blocks(degree * S))                                                              # :66
    cut_loss = torch.where(mask, -intra_edge_sum / (all_edge_sum + 1e-8), zero).sum() / live              # :69, live slots
    eye = torch.eye(K, dtype=torch.float32, device=dev)
    # a dead slot's S^T S is all zero, and the square root below has no derivative there: it takes the identity instead
    STS = torch.where(mask[:, None, None], blocks(S), eye)                                                # :76-80
    norm_STS = torch.sqrt(torch.sum(STS * STS, dim=(-2, -1), keepdim=True))                               # :82
    normed_STS = STS / (norm_STS + 1e-8)
    deviation = normed_STS - eye / float(np.sqrt(np.float32(K)))          # :86-87; a host scalar: nothing is uploaded
    orth = torch.sqrt(torch.sum(deviation * deviation, dim=(-2, -1)))
    orth_loss = torch.where(mask, orth, zero).sum() / live                                                # :89, live slots
    return cut_loss, orth_loss


def min_cut_pool_compute_losses_static(batch, dense_assign, normed_edge_weight=None):
    """(cut_loss, orth_loss) of nn.min_cut_pool_compute_losses on a static batch: the means over the LIVE slots, all on the
    device (a batch without live slots gives 0.0, 0.0).  Differentiable in dense_assign and in a normed_edge_weight that is
    passed in."""
    what = "min_cut_pool_compute_losses_static"
    car = _Carried(what, batch)
    S, K = _assign(what, car, dense_assign)
    if normed_edge_weight is None:
        normed_edge_weight = _normed_weight(what, car, batch.edge_weight)
    return _losses_static(car, S, K, L.as_f32(normed_edge_weight, car.dev).reshape(-1))


def min_cut_pool_static(x, batch, feature_gnn, assign_gnn, num_clusters, bias=None, activation=None, gnn_use_normed_edge=True,
                        return_loss_func=False, return_losses=False, training=None):
    """
    MinCutPool on a static batch (nn.min_cut_pool's arguments with `batch` for the four graph tensors).

    :return: the pooled StaticBatchGraph; with return_loss_func (pooled, loss_func), loss_func() -> (cut_loss, orth_loss); with
        return_losses (pooled, (cut_loss, orth_loss)).  The losses are means over the live slots.

    A batch.edge_weight that requires grad is refused (the normalisation is raw kernel launches), as nn.min_cut_pool does.
    With gnn_use_normed_edge the two GNNs get a cache of their own (the plan only): batch.cache may hold what another layer
    derived from the raw weights under a key that does not see the weights.
    """
    what = "min_cut_pool_static"
    if return_loss_func and return_losses:
        raise ValueError("return_loss_func and return_losses cannot be set to True at the same time")          # :179-180
    car = _Carried(what, batch)
    x = car.rows(what, "x", x)
    normed = _normed_weight(what, car, batch.edge_weight)                                                       # :190
    if gnn_use_normed_edge:
        gnn_weight, gnn_cache = normed, {CACHE_KEY_PLAN: car.plan}
    else:
        gnn_weight = batch.edge_weight
        if gnn_weight is None:
            gnn_weight = torch.ones(car.e_cap, dtype=torch.float32, device=car.dev)                             # :182-184
        gnn_cache = batch.cache
    inputs = [x, car.gnn_edge_index(), gnn_weight]
    assign_logits = assign_gnn(inputs, training=training, cache=gnn_cache)
    h = feature_gnn(inputs, training=training, cache=gnn_cache)
    S, K = _assign(what, car, torch.softmax(L.as_f32(assign_logits), dim=-1), num_clusters)                     # :204
    pooled = _coarsen_static(what, car, h, normed, S, K, True, bias=bias, activation=activation)
    if not (return_loss_func or return_losses):
        return pooled

    def loss_func():
        return _losses_static(car, S, K, normed)                                                                # :222-224

    if return_loss_func:
        return pooled, loss_func
    return pooled, loss_func()
