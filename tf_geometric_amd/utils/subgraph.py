# coding=utf-8
"""Node-induced subgraphs (BatchGraph.sample_new_graph_by_node_index, tf_geometric/data/graph.py:276-359) on the
device: the coarsening step of SAGPool / SortPool.

One host sync per call (tfgx_induced_subgraph_count returns the kept-edge count, and reports a duplicate or
out-of-range node id through the same read); the rest is asynchronous.  When the parent graph has a CSR plan, the
pooled graph's plan is derived from it without sorting and handed on as ``pooled_edge_index._tfgx_plan`` (picked up by
CsrPlan.from_cache and SparseMatrix.plan), so the next convolution does not sort again."""
import ctypes

import numpy as np
import torch

from .. import _lib as L


def _out(t, as_numpy):
    return t.cpu().numpy() if (as_numpy and t is not None) else t


def refuse_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("{} cannot run inside a hipGraph capture: the pooled graph's size depends on the data and is "
                           "read back to the host".format(what))


class InducedSubgraph(object):
    """node_map [n] (new id or -1), edge_index [2, E'] (kept edges in original order, relabelled), edge_id [E'] (their
    original ids), plan (the pooled graph's CsrPlan, or None without a parent plan)."""

    def __init__(self, node_map, edge_index, edge_id, plan):
        self.node_map = node_map
        self.edge_index = edge_index
        self.edge_id = edge_id
        self.plan = plan


def induced_subgraph(edge_index, node_index, num_nodes, parent_plan=None):
    """Keep the edges of `edge_index` whose endpoints are both in `node_index` (int32 device tensors; node_index
    without duplicates, every id in [0, num_nodes)); renumber them by position in node_index.  `parent_plan`: a CsrPlan
    of this edge list as an [num_nodes, num_nodes] operator, or None."""
    lib = L.require_gpu()
    ei = L.as_i32(edge_index)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    idx = L.as_i32(node_index, ei.device).reshape(-1)
    n, E, m = int(num_nodes), int(ei.shape[1]), int(idx.shape[0])
    dev = ei.device
    if parent_plan is not None:
        parent_plan = parent_plan.padded_to(n, n)
        if parent_plan is not None and parent_plan.num_edges != E:
            parent_plan = None
    with_plan = parent_plan is not None
    row, col = ei[0].contiguous(), ei[1].contiguous()
    node_map = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ws_bytes = lib.tfgx_induced_subgraph_workspace_bytes(n, E, m, int(with_plan))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    kept = ctypes.c_int64(0)
    L.check(lib.tfgx_induced_subgraph_count(L.ptr(row), L.ptr(col), E, n, L.ptr(idx), m, L.ptr(node_map),
                                            ctypes.byref(kept), L.ptr(ws), ws_bytes, L.stream_ptr()),
            "tfgx_induced_subgraph_count")
    K = int(kept.value)
    out = torch.empty((2, K), dtype=torch.int32, device=dev)
    edge_id = torch.empty(K, dtype=torch.int32, device=dev)
    row_ptr = plan_col = plan_perm = None
    if with_plan:
        row_ptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
        plan_col = torch.empty(K, dtype=torch.int32, device=dev)
        plan_perm = torch.empty(K, dtype=torch.int32, device=dev)
    L.check(lib.tfgx_induced_subgraph_emit(
        L.ptr(row), L.ptr(col), E, n, L.ptr(idx), m, L.ptr(node_map), K,
        L.ptr(parent_plan.row_ptr) if with_plan else None, L.ptr(parent_plan.col) if with_plan else None,
        L.ptr(parent_plan.perm) if with_plan else None, L.ptr(out[0]), L.ptr(out[1]), L.ptr(edge_id),
        L.ptr(row_ptr), L.ptr(plan_col), L.ptr(plan_perm), L.ptr(ws), ws_bytes, L.stream_ptr()),
        "tfgx_induced_subgraph_emit")
    plan = None
    if with_plan:
        from ..plan import CsrPlan
        plan = CsrPlan(row_ptr, plan_col, plan_perm, m, m, K)
        plan._edge_index = out
    return InducedSubgraph(node_map[:n], out, edge_id, plan)


def gather_i32(src, idx):
    """src[idx] for int32 device tensors (tfgx_gather_i32)."""
    lib = L.require_gpu()
    out = torch.empty(int(idx.shape[0]), dtype=torch.int32, device=src.device)
    L.check(lib.tfgx_gather_i32(L.ptr(src), L.ptr(idx), int(idx.shape[0]), L.ptr(out), L.stream_ptr()), "tfgx_gather_i32")
    return out


def gather_edge_attr(w, edge_id):
    """w[edge_id] for a 1-D edge attribute: the permute kernel, or a differentiable gather when w is being tracked."""
    from .. import autograd as AG
    w = L.as_f32(w)
    if AG.needs_grad(w):
        return AG.gather_edges(w, edge_id)
    return AG.gather_edge_values(w.reshape(-1), edge_id)


def parent_plan_of(edge_index, num_nodes, cache=None):
    """The CSR plan a pooling step derives the pooled plan from: the one attached to `edge_index` (a previous pooling,
    the neighbour sampler), else the one in `cache`, else a fresh build."""
    from ..plan import CsrPlan
    return CsrPlan.from_cache(edge_index, num_nodes, num_nodes, cache=cache)


def pool_graph(x, edge_index, edge_weight, node_graph_index, node_index, num_nodes, score=None, plan=None,
               x_numpy=False):
    """The pooled graph [x', edge_index', edge_weight', node_graph_index'] for kept nodes `node_index` (device int32):
    x' = (x * score)[node_index] as one differentiable gather-scale, the induced edge list with its derived plan attached,
    edge_weight' = edge_weight[kept edges] (None stays None), node_graph_index' = node_graph_index[node_index].  numpy in ->
    numpy out for the index / weight arrays (the reference's type rules)."""
    from .. import autograd as AG
    ei_np = not isinstance(edge_index, torch.Tensor)
    ei = L.as_i32(edge_index)
    E = int(ei.shape[1]) if ei.dim() == 2 else 0
    if x is not None and int(np.shape(x)[0]) != num_nodes:
        raise ValueError("x has {} rows, the graph has {} nodes".format(int(np.shape(x)[0]), num_nodes))
    if node_graph_index is not None and int(np.shape(node_graph_index)[0]) != num_nodes:
        raise ValueError("node_graph_index has {} entries, the graph has {} nodes".format(
            int(np.shape(node_graph_index)[0]), num_nodes))
    if edge_weight is not None and int(np.shape(edge_weight)[0]) != E:
        raise ValueError("edge_weight has {} entries, edge_index has {} edges".format(int(np.shape(edge_weight)[0]), E))
    sub = induced_subgraph(ei, node_index, num_nodes, parent_plan=plan)
    px = None
    if x is not None:
        px = AG.gather_scale(L.as_f32(x), node_index, sub.node_map, None if score is None else score)
        if x_numpy:
            px = px.detach().cpu().numpy()
    pw = None
    if edge_weight is not None:
        pw = _out(gather_edge_attr(edge_weight, sub.edge_id), not isinstance(edge_weight, torch.Tensor))
    pgi = None
    if node_graph_index is not None:
        pgi = _out(gather_i32(L.as_i32(node_graph_index), node_index), not isinstance(node_graph_index, torch.Tensor))
    pei = sub.edge_index
    if ei_np:
        pei = pei.cpu().numpy()
    elif sub.plan is not None:
        from ..plan import attach_plan
        attach_plan(pei, sub.plan)      # CsrPlan.from_cache / SparseMatrix.plan pick it up: no sort in the next layer
    return px, pei, pw, pgi


def compute_edge_mask_by_node_index(edge_index, node_index):
    """Bool mask of the edges whose two endpoints are in node_index (utils/graph_utils.py:538-551; duplicates allowed).
    numpy in -> numpy out."""
    as_np = not isinstance(edge_index, torch.Tensor)
    ei = L.as_i32(edge_index)
    idx = L.as_i32(node_index, ei.device).reshape(-1).long()
    hi = max(int(ei.max().item()) if ei.numel() else -1, int(idx.max().item()) if idx.numel() else -1) + 1
    node_mask = torch.zeros(max(hi, 1), dtype=torch.bool, device=ei.device)
    node_mask[idx] = True
    mask = node_mask[ei[0].long()] & node_mask[ei[1].long()]
    return _out(mask, as_np)


def sample_new_graph_by_node_index(edge_index, sampled_node_index, x=None, edge_weight=None, node_graph_index=None):
    """Functional form of BatchGraph.sample_new_graph_by_node_index (data/graph.py:276-359): returns
    (x, edge_index, edge_weight, node_graph_index) of the subgraph induced by `sampled_node_index`, nodes renumbered
    by their position in it (any order; duplicates are refused).  numpy in -> numpy out, tensor in -> tensor out."""
    refuse_capture("sample_new_graph_by_node_index")
    ei = L.as_i32(edge_index)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    idx = L.as_i32(sampled_node_index, ei.device).reshape(-1)
    if x is not None:
        n = int(np.shape(x)[0])
    elif node_graph_index is not None:
        n = int(np.shape(node_graph_index)[0])
    else:
        n = max(int(ei.max().item()) if ei.numel() else -1, int(idx.max().item()) if idx.numel() else -1) + 1
    from ..plan import attached_plan
    plan = attached_plan(edge_index)      # a pooled / sampled edge list hands its plan on
    return pool_graph(x, edge_index, edge_weight, node_graph_index, idx, n, plan=plan,
                      x_numpy=x is not None and not isinstance(x, torch.Tensor))
