# coding=utf-8
"""Node rows to the dense [G, k, F] tensor of a batch of graphs (include/tfgx_rows3d.h): utils.convert_x_to_3d and the fused
SortPool readout of DGCNN, sort_pool_3d, which goes from node rows straight to [G, k, F] in one launch with no edge work — on
ordinary batches and, without any host read, on StaticBatchGraph (sort_pool_static, rows_3d_static).

Reference: tf_geometric/utils/graph_utils.py:215-249 (convert_x_to_3d), tf_geometric/nn/pool/sort_pool.py:7-35 and
demo/demo_sort_pool.py:87-103 (SortPool(k) -> convert_x_to_3d -> Conv1D)."""
import numpy as np
import torch

from ... import _lib as L
from .common_pool import _graph_plan
from .topk_pool import topk_pool


def longest_graph(plan):
    """The longest row of a graph plan, kept on the plan (and so with the cache entry that holds it).  GraphStore.collate sets
    it from its host table; otherwise it is read from the device once, the first time it is asked for."""
    longest = getattr(plan, "_longest_row", None)
    if longest is None:
        longest = int(plan.in_degree().max().item()) if plan.n_dst > 0 else 0
        plan._longest_row = longest
    return longest


def _check_k(k, what):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("{}: k must be an integer of at least 1, got {!r}".format(what, k))
    return int(k)


def _sort_column(x, sort_index, what):
    F = int(x.shape[1])
    if isinstance(sort_index, bool) or not isinstance(sort_index, (int, np.integer)) or not -F <= sort_index < F:
        raise ValueError("{}: sort_index = {!r} is no column of x with {} features".format(what, sort_index, F))
    return int(sort_index) % F


def _features(x, what):
    if not hasattr(x, "shape") or len(x.shape) != 2:
        raise ValueError("{}: x must be [num_nodes, num_features], got shape {}".format(what, tuple(getattr(x, "shape", ()))))
    return L.as_f32(x)


def _ids_and_count(x, index, num, what):
    ids = L.as_i32(index, x.device).reshape(-1)
    n = int(ids.shape[0])
    if int(x.shape[0]) != n:
        raise ValueError("{}: x has {} rows, the index has {} entries".format(what, int(x.shape[0]), n))
    if num is None:
        if n == 0:
            raise ValueError("{}: no nodes and no count given: the first axis has no size".format(what))
        num = int(ids.max().item()) + 1                         # the reference's shape: max index of source + 1
    elif isinstance(num, bool) or not isinstance(num, (int, np.integer)) or num < 0:
        raise ValueError("{}: the count must be an integer of at least 0, got {!r}".format(what, num))
    return ids, n, int(num)


def convert_x_to_3d(x, source_index, k=None, pad=True, num_sources=None, cache=None):
    """
    Rows grouped by source -> the dense [num_sources, k, F] tensor (utils/graph_utils.py:215-249; the first four arguments are
    the reference's).  The nodes are grouped by `source_index`, stable; a node's slot is its position within its group; groups
    longer than k are cut off and shorter ones are zero-padded.

    :param k: slots per source.  None: the largest group.  With pad=False a k above the largest group shrinks to it.
    :param num_sources: the first axis; None: max(source_index) + 1
    :param cache: a batch's cache dict: the graph plan is taken from it, and kept there when it has to be built (the rule of
        the readouts, nn.mean_pool)
    :return: numpy in -> numpy out, tensor in -> tensor out; differentiable wrt x.

    Host reads, only where the reference's shape needs them: max(source_index) without num_sources, the largest group
    without k or with pad=False, and the graph-plan build on a cold cache.  With k, pad=True, num_sources and a warm cache
    there is none: one launch (tfgx_segment_rows_3d_f32, plain mode).
    """
    from ... import autograd as AG
    what = "convert_x_to_3d"
    as_np = not isinstance(x, torch.Tensor)
    xt = _features(x, what)
    ids, n, G = _ids_and_count(xt, source_index, num_sources, what)
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0):
        raise ValueError("{}: k must be None or an integer of at least 0, got {!r}".format(what, k))
    plan = _graph_plan(ids, G, n, cache) if G > 0 else None
    if k is None or not pad:
        largest = longest_graph(plan) if plan is not None else 0
        k = largest if k is None else min(int(k), largest)
    k, F = int(k), int(xt.shape[1])
    if G == 0 or k == 0:
        out = torch.zeros((G, k, F), dtype=torch.float32, device=xt.device)
    else:
        out = AG.segment_rows_3d(xt, plan.row_ptr, plan.col, G, n, k)[0].reshape(G, k, F)
    return out.detach().cpu().numpy() if as_np else out


def sort_pool_3d_route(node_graph_index, num_graphs=None, cache=None):
    """"fused" (one launch of tfgx_segment_rows_3d_f32 in its sort mode) or "composed" (topk_pool, the row gather, then the
    plain mode): what sort_pool_3d itself dispatches on.  A batch with a graph of more than L.ROWS3D_MAX_GRAPH_NODES nodes — the
    keys one workgroup ranks in LDS — is composed.  Builds (and caches) the graph plan like sort_pool_3d does."""
    ids = L.as_i32(node_graph_index).reshape(-1)
    n = int(ids.shape[0])
    if num_graphs is None:
        num_graphs = int(ids.max().item()) + 1 if n else 0
    if int(num_graphs) == 0:
        return "fused"
    return "fused" if longest_graph(_graph_plan(ids, int(num_graphs), n, cache)) <= L.ROWS3D_MAX_GRAPH_NODES else "composed"


def sort_pool_3d(x, node_graph_index, k=None, sort_index=-1, num_graphs=None, cache=None, return_index=False, ratio=None):
    """
    The SortPool readout of DGCNN: [num_graphs, k, F], graph g's nodes in descending order of column `sort_index`, cut off
    after k and zero-padded.  Bit for bit

        convert_x_to_3d(sort_pool(x, edge_index, w, node_graph_index, k=k, sort_index=sort_index)[0],
                        pooled_node_graph_index, k=k, num_sources=num_graphs)

    in ONE launch, without the pooled edge list that route builds and DGCNN never looks at.  The key is x.detach()[:,
    sort_index] (nn/pool/sort_pool.py:26): equal keys keep their order, -0.0 equals +0.0, NaNs go where topk_pool puts them.

    :param k: slots per graph, an int of at least 1 (ratio= has no 3-D form: ValueError)
    :param num_graphs: None: max(node_graph_index) + 1, read back
    :param cache: a batch's cache dict, for the graph plan (as in the readouts).  With it warm and num_graphs given there is
        no host read.
    :param return_index: also return slot_node int32 [num_graphs, k]: the node of every slot, -1 for padding
    :return: numpy in -> numpy out; differentiable wrt x (every row of dx is written once through the kernel's node_slot)
    """
    from ... import autograd as AG
    what = "sort_pool_3d"
    if ratio is not None:
        raise ValueError("{}: ratio= has no 3-D form (the second axis would depend on the data): give k".format(what))
    k = _check_k(k, what)
    as_np = not isinstance(x, torch.Tensor)
    xt = _features(x, what)
    ids, n, G = _ids_and_count(xt, node_graph_index, num_graphs, what)
    F = int(xt.shape[1])
    if F == 0:
        raise ValueError("{}: x has no column to sort by".format(what))
    col = _sort_column(xt, sort_index, what)
    if G == 0:
        out = torch.zeros((0, k, F), dtype=torch.float32, device=xt.device)
        slot_node = torch.zeros((0, k), dtype=torch.int32, device=xt.device)
    else:
        plan = _graph_plan(ids, G, n, cache)
        if longest_graph(plan) <= L.ROWS3D_MAX_GRAPH_NODES:
            out, slot_node, _ = AG.segment_rows_3d(xt, plan.row_ptr, plan.col, G, n, k, sort_col=col)
        else:
            out, slot_node = _composed(xt, ids, plan, G, n, k, col)
        out, slot_node = out.reshape(G, k, F), slot_node.reshape(G, k)
    if as_np:
        out, slot_node = out.detach().cpu().numpy(), slot_node.cpu().numpy()
    return (out, slot_node) if return_index else out


def _composed(xt, ids, plan, G, n, k, col):
    """The route of a batch with a graph above the LDS cap: topk_pool's global sort (one host read), the differentiable row
    gather of sort_pool, then the plain mode over the pooled rows, whose graph g holds min(n_g, k) of them."""
    from ... import autograd as AG
    dev = xt.device
    node_index = topk_pool(ids, xt.detach()[:, col], k=k, num_segments=G)
    m = int(node_index.shape[0])
    node_map = torch.full((n,), -1, dtype=torch.int32, device=dev)
    node_map[node_index.long()] = torch.arange(m, dtype=torch.int32, device=dev)
    pooled = AG.gather_scale(xt, node_index, node_map)
    seg_ptr = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    seg_ptr[1:] = torch.cumsum(plan.in_degree().clamp(max=k), 0)
    out, slot, _ = AG.segment_rows_3d(pooled, seg_ptr, None, G, m, k)
    slot_node = torch.where(slot >= 0, node_index[slot.clamp(min=0).long()], slot) if m else slot
    return out, slot_node


def _static(x, batch, what):
    from .sag_pool_static import _static_batch
    _static_batch(batch, what)          # refuses a non-static batch and a store whose largest graph exceeds the cap, by name
    n_cap = batch.capacities.n_cap
    if not hasattr(x, "shape") or len(x.shape) != 2 or int(x.shape[0]) != n_cap:
        raise ValueError("{}: x must have one row per row of the batch ([{}, F]), got shape {}".format(
            what, n_cap, tuple(getattr(x, "shape", ()))))
    return L.as_f32(x, batch.edge_index.device), batch.capacities.batch_size, n_cap


def sort_pool_static(x, batch, k, sort_index=-1, return_index=False):
    """sort_pool_3d on a StaticBatchGraph — GraphStore.collate_static's, or a sag_pool_static output: [B, k, F], slot for slot
    what sort_pool_3d gives on collate(live ids), the rows of dead slots exactly zero.  It runs over batch.graph_row_ptr with
    the B slots as the graphs, so the dead graph B and every padded row are never read.  No host read: capturable.  The
    kernel's flag word is ORed into batch.counts[3] on the device (StaticBatchGraph.check names TOO_LONG)."""
    from ... import autograd as AG
    what = "sort_pool_static"
    k = _check_k(k, what)
    xt, B, n_cap = _static(x, batch, what)
    F = int(xt.shape[1])
    if F == 0:
        raise ValueError("{}: x has no column to sort by".format(what))
    col = _sort_column(xt, sort_index, what)
    if B == 0:
        out, slot_node = xt.new_zeros((0, k, F)), torch.zeros((0, k), dtype=torch.int32, device=xt.device)
    else:
        out, slot_node, flags = AG.segment_rows_3d(xt, batch.graph_row_ptr, None, B, n_cap, k, sort_col=col)
        batch.counts[3:4].bitwise_or_(flags)
        out, slot_node = out.reshape(B, k, F), slot_node.reshape(B, k)
    return (out, slot_node) if return_index else out


def rows_3d_static(h, batch, k):
    """convert_x_to_3d on a StaticBatchGraph (StaticBatchGraph.to_3d): [B, k, F], slot j of graph g its j-th row; graphs
    longer than k are cut off, the rest — dead slots included — is exactly zero.  No host read: capturable."""
    from ... import autograd as AG
    what = "StaticBatchGraph.to_3d"
    k = _check_k(k, what)
    xt, B, n_cap = _static(h, batch, what)
    F = int(xt.shape[1])
    if B == 0:
        return xt.new_zeros((0, k, F))
    return AG.segment_rows_3d(xt, batch.graph_row_ptr, None, B, n_cap, k)[0].reshape(B, k, F)
