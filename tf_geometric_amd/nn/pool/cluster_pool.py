# coding=utf-8
"""cluster_pool (reference: tf_geometric/nn/pool/cluster_pool.py:9-46): coarsen a graph by a sparse node -> cluster
assignment S: pooled adjacency S^T A S, pooled features S^T x.

The reference densifies A ([N, N]) and scans a dense [K, K] result.  Here S^T A S is a sparse product by expand - sort -
compress (tfgx_spasp_count / _emit / _reduce, include/tfgx_asap.h): every edge (u, v) of A meets every cluster of u and every
cluster of v, the products are sorted by (row cluster, column cluster) and each run is summed in order.  No [N, N] or [K, K]
tensor exists; clusters may span graphs.  Two host reads per call: the size of the expansion and the pooled edge count."""
import ctypes

import numpy as np
import torch

from ... import _lib as L
from ... import autograd as AG
from ...plan import CsrPlan, segment_reduce
from ...utils.subgraph import refuse_capture


def sparse_sas(s_row_ptr, s_col, s_val, num_nodes, num_clusters, a_row, a_col, a_val, drop_diagonal=False):
    """P = S^T A S for S in CSR by node (int32 s_row_ptr [N + 1], s_col [nnz], float32 s_val or None = ones; an entry whose
    cluster id is outside [0, K) does not belong to S) and A as an edge list (int32 a_row / a_col [E], float32 a_val or None).
    -> (row [nnz], col [nnz], val [nnz], row_ptr [K + 1]): the entries != 0.0 sorted by (row, col), without the diagonal
    when drop_diagonal.  Device tensors in and out."""
    lib = L.require_gpu()
    N, K, E = int(num_nodes), int(num_clusters), int(a_row.shape[0])
    dev = a_row.device
    s_deg = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    offsets = torch.empty(E + 1, dtype=torch.int64, device=dev)
    ws_bytes = lib.tfgx_spasp_count_workspace_bytes(N, E)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    total = ctypes.c_int64(0)
    L.check(lib.tfgx_spasp_count(L.ptr(s_row_ptr), L.ptr(s_col), N, K, L.ptr(a_row), L.ptr(a_col), E, L.ptr(s_deg),
                                 L.ptr(offsets), ctypes.byref(total), L.ptr(ws), ws_bytes, L.stream_ptr()), "tfgx_spasp_count")
    T = int(total.value)
    ws_bytes = lib.tfgx_spasp_workspace_bytes(T, K)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.tfgx_spasp_emit(L.ptr(s_row_ptr), L.ptr(s_col), L.ptr(s_val), N, K, L.ptr(a_row), L.ptr(a_col), L.ptr(a_val), E,
                                L.ptr(s_deg), L.ptr(offsets), T, L.ptr(ws), ws_bytes, L.stream_ptr()), "tfgx_spasp_emit")
    out_row = torch.empty(T, dtype=torch.int32, device=dev)
    out_col = torch.empty(T, dtype=torch.int32, device=dev)
    out_val = torch.empty(T, dtype=torch.float32, device=dev)
    row_ptr = torch.empty(K + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.tfgx_spasp_reduce(T, K, int(bool(drop_diagonal)), L.ptr(out_row), L.ptr(out_col), L.ptr(out_val),
                                  L.ptr(row_ptr), L.ptr(count), L.ptr(ws), ws_bytes, L.stream_ptr()), "tfgx_spasp_reduce")
    nnz = int(count.item())
    return out_row[:nnz], out_col[:nnz], out_val[:nnz], row_ptr


def cluster_pool(x, edge_index, edge_weight, assign_edge_index, assign_edge_weight, num_clusters, num_nodes=None):
    """
    Coarsen the input graph by a cluster assignment of its nodes (same arguments as the reference).

    :param x: [num_nodes, num_features] node features, or None
    :param edge_index: [2, num_edges]
    :param edge_weight: [num_edges] or None (ones)
    :param assign_edge_index: [2, num_assignments] = [node id; cluster id]: S[node, cluster] (duplicates add up)
    :param assign_edge_weight: [num_assignments] or None (ones)
    :param num_clusters: number of clusters K
    :param num_nodes: number of nodes; required when x is None
    :return: [pooled_x, pooled_edge_index, pooled_edge_weight]: pooled_x = S^T x ([K, F], None when x is None); the entries
        != 0.0 of S^T A S in row-major order, the diagonal included (int32 [2, nnz], float32 [nnz]).  numpy in -> numpy out
        for the edge list.

    pooled_x is differentiable with respect to x.  The pooled adjacency is NOT differentiable: because the adjacency is
    always returned, an edge_weight or assign_edge_weight that requires grad raises NotImplementedError (detach it; ASAP's
    assignment is detached by definition).
    """
    refuse_capture("cluster_pool")
    L.require_gpu()
    if num_nodes is None:
        if x is None:
            raise Exception("Please provide num_nodes if x is None")          # cluster_pool.py:25-27
        num_nodes = int(np.shape(x)[0])
    if AG.needs_grad(edge_weight, assign_edge_weight):
        raise NotImplementedError("cluster_pool: the pooled adjacency S^T A S is not differentiable; edge_weight and "
                                  "assign_edge_weight must not require grad (detach them)")
    N, K = int(num_nodes), int(num_clusters)
    as_np = not isinstance(edge_index, torch.Tensor)
    ei = L.as_i32(edge_index)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    dev = ei.device
    aei = L.as_i32(assign_edge_index, dev)
    if aei.numel() == 0:
        aei = aei.reshape(2, 0)
    a_val = None if edge_weight is None else L.as_f32(edge_weight, dev).reshape(-1).contiguous()
    aw = None if assign_edge_weight is None else L.as_f32(assign_edge_weight, dev).reshape(-1).contiguous()
    s_plan = CsrPlan.build(aei, N, max(K, 1))          # S by node: row_ptr over nodes, col = cluster ids (validated here)
    s_val = s_plan.edge_attr_to_csr(aw)
    row, col, val, _ = sparse_sas(s_plan.row_ptr, s_plan.col, s_val, N, K, ei[0].contiguous(), ei[1].contiguous(), a_val)
    pooled_edge_index = torch.stack([row, col])
    pooled_x = None
    if x is not None:
        xf = L.as_f32(x, dev)
        st_plan = CsrPlan.build(torch.stack([aei[1], aei[0]]), K, N)      # S^T by cluster
        st_val = st_plan.edge_attr_to_csr(aw)
        if AG.needs_grad(xf):
            pooled_x = AG.aggregate(st_plan, xf, L.SUM, w_csr=st_val)
        else:
            pooled_x = segment_reduce(st_plan, xf, L.SUM, w_csr=st_val)
    if as_np:
        return pooled_x, pooled_edge_index.cpu().numpy(), val.cpu().numpy()
    return pooled_x, pooled_edge_index, val
