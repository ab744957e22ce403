# coding=utf-8
"""float64 torch restatement of the reference's DiffPool and MinCutPool, line for line (nn/pool/diff_pool.py:8-105,
nn/pool/min_cut_pool.py:18-232, nn/pool/cluster_pool.py:32-46): the dense assignment becomes a [N, G K] matrix, the adjacency
a dense [N, N] one, S^T A S and S^T x dense products, the pooled edges the row-major non-zeros.  CPU tensors, small sizes,
differentiable by torch autograd.  The two GNNs are GCN layers with given weights (norm both, renormalised, unit self-loops:
the reference's gcn on an edge list without self-loops), or any callable (x, row, col, wv) -> tensor.

absolute=True keeps every forward value and back-propagates |cotangent| through |local Jacobians| (asap_mirror._Ops), which
yields the sum of |terms| of every gradient entry: the scale of the float32 error bar of tests/test_gpu_densepool.py.

tests/test_densepool_reference.py holds this mirror to the reference's own outputs (tests/golden/densepool_cases.npz)."""
import numpy as np
import torch

from asap_mirror import _Ops, _seg_sum, _t, edges_of


def _edges(edge_index):
    ei = np.asarray(edge_index).reshape(2, -1).astype(np.int64)
    return torch.from_numpy(ei[0]), torch.from_numpy(ei[1])


def gcn_mirror(ops, x, row, col, wv, kernel, bias):
    """gcn(x, SparseMatrix(edge_index, wv), kernel, bias): D^-1/2 (A + I) D^-1/2 x W + b, D = row sums of A + I."""
    n = int(x.shape[0])
    deg = _seg_sum(row, wv, n) + 1.0
    dis = deg.pow(-0.5)
    xw = ops.mm(x, kernel)
    h = _seg_sum(row, (dis[row] * wv * dis[col]).unsqueeze(1) * xw[col], n) + xw / deg.unsqueeze(1)
    return h if bias is None else h + bias


def adj_norm_edge_mirror(row, col, wv, n):
    """graph_utils.py:914-943 with add_self_loop=False: D^-1/2 A D^-1/2 on the edge list, inf / nan -> 0."""
    deg = _seg_sum(row, wv, n)
    dis = deg.pow(-0.5)
    dis = torch.where(torch.isinf(dis) | torch.isnan(dis), torch.zeros_like(dis), dis)
    return dis[row] * wv * dis[col]


def softmax_mirror(ops, z):
    ex = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())
    return ops.div(ex, ex.sum(dim=1, keepdim=True))


def _dense_assign(S, gid, G):
    """convert_dense_assign_to_edge + SparseMatrix: column j of node i is cluster K gid[i] + j (graph_utils.py:287-322)."""
    n, K = int(S.shape[0]), int(S.shape[1])
    rows = torch.arange(n).unsqueeze(1).expand(n, K)
    cols = gid.unsqueeze(1) * K + torch.arange(K).unsqueeze(0)
    return torch.zeros((n, G * K), dtype=S.dtype).index_put((rows, cols), S, accumulate=True)


def coarsen_mirror(ops, x, row, col, wv, gid, S, G, drop_diagonal=False):
    """cluster_pool on the [N, G K] assignment (cluster_pool.py:32-46) and, for MinCutPool, remove_self_loop_edge
    (min_cut_pool.py:143).  -> dict(x, edge_index, edge_weight, node_graph_index, P, P_abs, x_abs)."""
    n, K = int(S.shape[0]), int(S.shape[1])
    Sf = _dense_assign(S, gid, G)
    A = torch.zeros((n, n), dtype=S.dtype).index_put((row, col), wv, accumulate=True)
    P = ops.mm(ops.mm(Sf.t(), A), Sf)
    pei, pw = edges_of(P, drop_diagonal=drop_diagonal)
    px = None if x is None else ops.mm(Sf.t(), x)
    with torch.no_grad():
        P_abs = Sf.abs().t() @ A.abs() @ Sf.abs()
        x_abs = None if x is None else Sf.abs().t() @ x.abs()
    return dict(x=px, edge_index=pei, edge_weight=pw, node_graph_index=np.repeat(np.arange(G, dtype=np.int32), K), P=P,
                P_abs=P_abs, x_abs=x_abs)


def losses_mirror(ops, row, col, wn, gid, S, G):
    """min_cut_pool_compute_losses (min_cut_pool.py:28-90) for the normalised weights wn."""
    n, K = int(S.shape[0]), int(S.shape[1])
    degree = _seg_sum(row, wn, n)                                                                  # :29
    Sf = _dense_assign(S, gid, G)
    A = torch.zeros((n, n), dtype=S.dtype).index_put((row, col), wn, accumulate=True)
    diag = lambda M: torch.diagonal(M).reshape(-1, K).sum(dim=-1)                                  # noqa: E731   :11-14
    intra_edge_sum = diag(ops.mm(ops.mm(Sf.t(), A), Sf))                                           # :64
    all_edge_sum = diag(ops.mm(Sf.t(), degree.unsqueeze(1) * Sf))                                  # :66
    cut = torch.mean(ops.div(ops.mul(intra_edge_sum, torch.tensor(-1.0, dtype=S.dtype)), all_edge_sum + 1e-8))     # :69
    STS = ops.mm(Sf.t(), Sf)                                                                       # :76
    STS = ops.mm(STS, torch.eye(K, dtype=S.dtype).repeat(G, 1)).reshape(-1, K, K)                  # :78-80
    norm_STS = torch.sqrt(torch.sum(ops.mul(STS, STS), dim=(-2, -1), keepdim=True))                # :82
    normed_STS = ops.div(STS, norm_STS + 1e-8)                                                     # :84
    deviation = ops.sub(normed_STS, torch.eye(K, dtype=S.dtype) / float(np.sqrt(np.float32(K))))   # :86-87
    orth = torch.mean(torch.sqrt(torch.sum(ops.mul(deviation, deviation), dim=(-2, -1))))          # :89
    return cut, orth


def _gnn(ops, spec, x, row, col, wv):
    if callable(spec):
        return spec(ops, x, row, col, wv)
    kernel, bias = spec
    return gcn_mirror(ops, x, row, col, wv, kernel, bias)


def _finish(ops, out, bias, activation):
    if bias is not None:
        out["x"] = out["x"] + bias
    if activation == "relu":
        out["x"] = torch.relu(out["x"])
    elif activation is not None:
        out["x"] = activation(out["x"])
    return out


def diff_pool_coarsen_mirror(x, edge_index, edge_weight, gid, dense_assign, num_graphs=None, dtype=torch.float64,
                             absolute=False):
    ops = _Ops(absolute)
    row, col = _edges(edge_index)
    gid_t = torch.from_numpy(np.asarray(gid).astype(np.int64))
    G = int(gid_t.max()) + 1 if num_graphs is None else int(num_graphs)
    wv = torch.ones(int(row.shape[0]), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)
    return coarsen_mirror(ops, _t(x, dtype), row, col, wv, gid_t, _t(dense_assign, dtype), G)


def diff_pool_mirror(x, edge_index, edge_weight, gid, feature_gnn, assign_gnn, bias=None, activation=None, num_graphs=None,
                     dtype=torch.float64, absolute=False):
    """feature_gnn / assign_gnn: (kernel, bias) of a GCN, or a callable (ops, x, row, col, wv) -> tensor."""
    ops = _Ops(absolute)
    x = _t(x, dtype)
    row, col = _edges(edge_index)
    gid_t = torch.from_numpy(np.asarray(gid).astype(np.int64))
    G = int(gid_t.max()) + 1 if num_graphs is None else int(num_graphs)
    wv = torch.ones(int(row.shape[0]), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)      # :78-80
    logits = _gnn(ops, assign_gnn, x, row, col, wv)
    h = _gnn(ops, feature_gnn, x, row, col, wv)
    S = softmax_mirror(ops, logits)                                                                          # :92
    out = coarsen_mirror(ops, h, row, col, wv, gid_t, S, G)
    out["assign"] = S
    out["logits"] = logits
    return _finish(ops, out, bias, activation)


def min_cut_losses_mirror(edge_index, edge_weight, gid, dense_assign, num_graphs=None, dtype=torch.float64, absolute=False):
    ops = _Ops(absolute)
    row, col = _edges(edge_index)
    gid_t = torch.from_numpy(np.asarray(gid).astype(np.int64))
    G = int(gid_t.max()) + 1 if num_graphs is None else int(num_graphs)
    S = _t(dense_assign, dtype)
    wv = torch.ones(int(row.shape[0]), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)
    return losses_mirror(ops, row, col, adj_norm_edge_mirror(row, col, wv, int(S.shape[0])), gid_t, S, G)


def min_cut_pool_coarsen_mirror(x, edge_index, edge_weight, gid, dense_assign, num_graphs=None, dtype=torch.float64,
                                absolute=False):
    ops = _Ops(absolute)
    row, col = _edges(edge_index)
    gid_t = torch.from_numpy(np.asarray(gid).astype(np.int64))
    G = int(gid_t.max()) + 1 if num_graphs is None else int(num_graphs)
    S = _t(dense_assign, dtype)
    wv = torch.ones(int(row.shape[0]), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)
    wn = adj_norm_edge_mirror(row, col, wv, int(S.shape[0]))                                                 # :127-128
    return coarsen_mirror(ops, _t(x, dtype), row, col, wn, gid_t, S, G, drop_diagonal=True)


def min_cut_pool_mirror(x, edge_index, edge_weight, gid, feature_gnn, assign_gnn, bias=None, activation=None,
                        gnn_use_normed_edge=True, num_graphs=None, dtype=torch.float64, absolute=False):
    ops = _Ops(absolute)
    x = _t(x, dtype)
    n = int(x.shape[0])
    row, col = _edges(edge_index)
    gid_t = torch.from_numpy(np.asarray(gid).astype(np.int64))
    G = int(gid_t.max()) + 1 if num_graphs is None else int(num_graphs)
    wv = torch.ones(int(row.shape[0]), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)      # :182-184
    wn = adj_norm_edge_mirror(row, col, wv, n)                                                               # :190
    gw = wn if gnn_use_normed_edge else wv
    logits = _gnn(ops, assign_gnn, x, row, col, gw)
    h = _gnn(ops, feature_gnn, x, row, col, gw)
    S = softmax_mirror(ops, logits)                                                                          # :204
    out = coarsen_mirror(ops, h, row, col, wn, gid_t, S, G, drop_diagonal=True)
    out = _finish(ops, out, bias, activation)
    out["assign"] = S
    out["logits"] = logits
    out["cut_loss"], out["orth_loss"] = losses_mirror(ops, row, col, wn, gid_t, S, G)
    return out
