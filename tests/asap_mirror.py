# coding=utf-8
"""float64 torch mirror of ASAP and cluster_pool, written from the semantics of nn/pool/asap.py's docstring (reference
asap.py:19-131 with its two repairs: the current gcn signature and [node; cluster] assignment rows).  CPU tensors, dense
S^T A S (the sizes here are small), differentiable by torch autograd.  `topk_node_index=` forces the selection, so a test
can take the product's own choice and compare everything else; `keep_scale=` (a callable: int64 positions -> float64
multipliers) restates dropout, the position of an edge being its place in the stable sort of the self-loop-free list by row,
and num_edges + i for the self edge of node i.

tests/test_asap_reference.py holds this mirror to the reference's own outputs (tests/golden/asap_cases.npz);
tests/test_gpu_asap.py holds the product to the mirror."""
import numpy as np
import torch

WEIGHT_NAMES = ["attention_gcn_kernel", "attention_gcn_bias", "attention_query_kernel", "attention_query_bias",
                "attention_score_kernel", "attention_score_bias", "le_conv_self_kernel", "le_conv_self_bias",
                "le_conv_aggr_self_kernel", "le_conv_aggr_self_bias", "le_conv_aggr_neighbor_kernel"]


def make_weights(rng, F, A, scale=1.0):
    """The eleven weights as float32 numpy arrays (biases non-zero, so that they matter)."""
    def mat(a, b):
        return (rng.uniform(-1, 1, size=(a, b)) * np.sqrt(6.0 / (a + b)) * scale).astype(np.float32)

    def vec(a):
        return (rng.uniform(-0.3, 0.3, size=a)).astype(np.float32)
    return dict(attention_gcn_kernel=mat(F, A), attention_gcn_bias=vec(A), attention_query_kernel=mat(A, A),
                attention_query_bias=vec(A), attention_score_kernel=mat(2 * A, 1), attention_score_bias=vec(1),
                le_conv_self_kernel=mat(F, 1), le_conv_self_bias=vec(1), le_conv_aggr_self_kernel=mat(F, 1),
                le_conv_aggr_self_bias=vec(1), le_conv_aggr_neighbor_kernel=mat(F, 1))


def _t(a, dtype=torch.float64):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(dtype)
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _seg_sum(rows, vals, n):
    shape = (n,) + tuple(vals.shape[1:])
    return torch.zeros(shape, dtype=vals.dtype).index_add(0, rows, vals)


def _seg_max(rows, vals, n):
    out = torch.full((n,) + tuple(vals.shape[1:]), -float("inf"), dtype=vals.dtype)
    idx = rows.reshape(-1, *([1] * (vals.dim() - 1))).expand_as(vals)
    return out.scatter_reduce(0, idx, vals, reduce="amax", include_self=True)


def topk_select(gid, score, k=None, ratio=None):
    """topk_pool: graphs ascending, scores descending, ties in input order; ceil(float32(count) * float32(ratio))."""
    gid = np.asarray(gid)
    score = np.asarray(score, np.float64).reshape(-1)
    out = []
    for g in np.unique(gid):
        nodes = np.flatnonzero(gid == g)
        order = nodes[np.argsort(-score[nodes], kind="stable")]
        cnt = nodes.size
        nk = min(int(k), cnt) if k is not None else min(cnt, int(np.ceil(np.float32(cnt) * np.float32(ratio))))
        out.append(order[:nk])
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def dense_sas(n, K, a_row, a_col, a_val, s_node, s_cluster, s_val):
    """S^T A S as a dense [K, K] matrix of a_val's dtype (duplicates of A and of S add up)."""
    S = torch.zeros((n, K), dtype=a_val.dtype).index_put((s_node, s_cluster), s_val, accumulate=True)
    Adj = torch.zeros((n, n), dtype=a_val.dtype).index_put((a_row, a_col), a_val, accumulate=True)
    return S.t() @ Adj @ S


def edges_of(P, drop_diagonal=False):
    """Row-major entries != 0 of a dense matrix -> (int32 [2, nnz], values)."""
    mask = P != 0.0
    if drop_diagonal:
        mask = mask & ~torch.eye(P.shape[0], dtype=torch.bool)
    idx = torch.nonzero(mask)
    return idx.t().to(torch.int32).numpy().reshape(2, -1), P[idx[:, 0], idx[:, 1]]


class _AbsMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return a * b

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return g.abs() * b.abs(), g.abs() * a.abs()


class _AbsMatmul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return a @ b

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return g.abs() @ b.abs().t(), a.abs().t() @ g.abs()


class _AbsSub(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return a - b

    @staticmethod
    def backward(ctx, g):
        return g.abs(), g.abs()


class _AbsDiv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return a / b

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return g.abs() / b.abs(), g.abs() * a.abs() / (b * b)


class _Ops(object):
    """The four primitives of the mirror whose local Jacobian can be negative.  absolute=True keeps every forward value
    and replaces each of these backward rules by its absolute value; every other primitive used here (gather, segment sum,
    segment max, add, exp, leaky_relu, sigmoid, products with positive constants) has a non-negative Jacobian.  Back-propagating
    |cotangent| then yields, for every leaf entry, the sum over all paths of |product of local Jacobians| |cotangent|: the
    sum of |terms| of that gradient entry (for a function linear in its inputs this is the restatement on absolute values of
    tests/test_gpu_fuzz_backward.py)."""

    def __init__(self, absolute):
        self.absolute = absolute

    def mul(self, a, b):
        a, b = torch.broadcast_tensors(a, b)
        return _AbsMul.apply(a, b) if self.absolute else a * b

    def mm(self, a, b):
        return _AbsMatmul.apply(a, b) if self.absolute else a @ b

    def sub(self, a, b):
        a, b = torch.broadcast_tensors(a, b)
        return _AbsSub.apply(a, b) if self.absolute else a - b

    def div(self, a, b):
        a, b = torch.broadcast_tensors(a, b)
        return _AbsDiv.apply(a, b) if self.absolute else a / b


def asap_mirror(x, edge_index, edge_weight, gid, weights, k=None, ratio=None, activation="sigmoid", topk_node_index=None,
                keep_scale=None, dtype=torch.float64, absolute=False):
    """absolute=True: same values, but backward yields the sum of |terms| of every gradient entry (see _Ops).
    dtype=torch.float32 runs the same statements in float32 (a measure of what float32 arithmetic can reach).
    -> dict(cluster_h, node_score, idx, x, edge_index, edge_weight, node_graph_index, P (dense, off-diagonal + diagonal),
    p (per ei1 edge, after dropout)).  `weights`: name -> tensor / array (float64 leaves keep their autograd edge)."""
    ops = _Ops(absolute)
    x = _t(x, dtype)
    n = int(x.shape[0])
    W = {name: _t(weights.get(name), dtype) for name in WEIGHT_NAMES}
    ei = np.asarray(edge_index).reshape(2, -1)
    keep = ei[0] != ei[1]
    row = torch.from_numpy(ei[0][keep].astype(np.int64))
    col = torch.from_numpy(ei[1][keep].astype(np.int64))
    E0 = int(row.shape[0])
    w0 = None if edge_weight is None else _t(np.asarray(edge_weight)[keep], dtype)
    wv = torch.ones(E0, dtype=dtype) if w0 is None else w0
    ar = torch.arange(n)
    row1, col1 = torch.cat([row, ar]), torch.cat([col, ar])
    # 2. attention features: GCN (norm both, renormalised, symmetric; gcn.py:32-130)
    deg = _seg_sum(row, wv, n) + 1.0
    dis = deg.pow(-0.5)
    xw = ops.mm(x, W["attention_gcn_kernel"])
    h = _seg_sum(row, (dis[row] * wv * dis[col]).unsqueeze(1) * xw[col], n) + xw / deg.unsqueeze(1) + W["attention_gcn_bias"]
    # 3. master query
    q = ops.mm(_seg_max(row1, h[col1], n), W["attention_query_kernel"]) + W["attention_query_bias"]
    # 4. scores and the per-row softmax
    z = ops.mm(torch.cat([q[row1], h[col1]], dim=1), W["attention_score_kernel"]) + W["attention_score_bias"]
    s = torch.nn.functional.leaky_relu(z.reshape(-1), 0.2)
    m = _seg_max(row1, s.detach(), n)
    ex = torch.exp(s - m[row1])
    p = ops.div(ex, (_seg_sum(row1, ex, n) + 1e-8)[row1])
    # 5. dropout by position
    if keep_scale is not None:
        order = torch.argsort(row, stable=True)
        pos = torch.empty(E0, dtype=torch.int64)
        pos[order] = torch.arange(E0)
        p = p * _t(keep_scale(torch.cat([pos, E0 + ar])), dtype)
    # 6. cluster features
    c = _seg_sum(row1, ops.mul(p.unsqueeze(1), x[col1]), n)
    # 7. LEConv, literally (both gathered terms by col)
    def dense(kname, bname):
        out = ops.mm(c, W[kname])
        return out if W.get(bname) is None else out + W[bname]
    diff = ops.sub(dense("le_conv_aggr_self_kernel", "le_conv_aggr_self_bias"), dense("le_conv_aggr_neighbor_kernel", "none"))
    score = dense("le_conv_self_kernel", "le_conv_self_bias") + _seg_sum(row, wv.unsqueeze(1) * diff[col], n)
    # 8. selection
    gid_np = np.asarray(gid).reshape(-1)
    idx = topk_select(gid_np, score.detach().numpy(), k, ratio) if topk_node_index is None \
        else np.asarray(topk_node_index, np.int64).reshape(-1)
    K = int(idx.shape[0])
    idx_t = torch.from_numpy(idx)
    # 9. pooled features
    ts = score[idx_t]
    if activation == "sigmoid":
        ts = torch.sigmoid(ts)
    elif activation is not None:
        ts = activation(ts)
    pooled_x = ops.mul(c[idx_t], ts)
    # 10. S^T A1 S with the detached assignment
    node_map = torch.full((n,), -1, dtype=torch.int64)
    node_map[idx_t] = torch.arange(K)
    cl = node_map[row1]
    sel = cl >= 0
    a1 = torch.cat([wv.detach(), torch.ones(n, dtype=dtype)])
    P = dense_sas(n, K, row1, col1, a1, col1[sel], cl[sel], p.detach()[sel])
    # 11. off-diagonal entries, then the unit diagonal
    pei, pw = edges_of(P, drop_diagonal=True)
    ark = np.arange(K, dtype=np.int32)
    pei = np.concatenate([pei, np.stack([ark, ark])], axis=1).astype(np.int32)
    pw = torch.cat([pw, torch.ones(K, dtype=dtype)])
    # |terms| of every entry of P: the same product on absolute values (the bar of the aggregation tests)
    P_abs = dense_sas(n, K, row1, col1, a1.abs(), col1[sel], cl[sel], p.detach()[sel].abs())
    # sum |terms| of the two aggregations in front of pooled_x (for the sqrt bar of the aggregation tests)
    with torch.no_grad():
        c_abs = _seg_sum(row1, p.abs().unsqueeze(1) * x.abs()[col1], n)

        def dense_abs(kname, bname):
            out = c.abs() @ W[kname].abs()
            return out if W.get(bname) is None else out + W[bname].abs()
        diff_abs = dense_abs("le_conv_aggr_self_kernel", "le_conv_aggr_self_bias") + dense_abs("le_conv_aggr_neighbor_kernel", "none")
        score_abs = dense_abs("le_conv_self_kernel", "le_conv_self_bias") + _seg_sum(row, wv.unsqueeze(1) * diff_abs[col], n)
    return dict(cluster_h=c, node_score=score, idx=idx, c_abs=c_abs, score_abs=score_abs, pooled_score=ts, x=pooled_x, edge_index=pei, edge_weight=pw,
                node_graph_index=gid_np[idx], P=P, P_abs=P_abs, p=p, row1=row1, col1=col1)


def cluster_pool_mirror(x, edge_index, edge_weight, assign_edge_index, assign_edge_weight, num_clusters, num_nodes=None):
    if num_nodes is None:
        if x is None:
            raise Exception("Please provide num_nodes if x is None")
        num_nodes = int(np.shape(x)[0])
    n, K = int(num_nodes), int(num_clusters)
    ei = torch.from_numpy(np.asarray(edge_index).reshape(2, -1).astype(np.int64))
    aei = torch.from_numpy(np.asarray(assign_edge_index).reshape(2, -1).astype(np.int64))
    a = torch.ones(ei.shape[1], dtype=torch.float64) if edge_weight is None else _t(edge_weight)
    sv = torch.ones(aei.shape[1], dtype=torch.float64) if assign_edge_weight is None else _t(assign_edge_weight)
    P = dense_sas(n, K, ei[0], ei[1], a, aei[0], aei[1], sv)
    P_abs = dense_sas(n, K, ei[0], ei[1], a.abs(), aei[0], aei[1], sv.abs())
    pei, pw = edges_of(P)
    px = None
    if x is not None:
        px = torch.zeros((n, K), dtype=torch.float64).index_put((aei[0], aei[1]), sv, accumulate=True).t() @ _t(x)
    return dict(x=px, edge_index=pei, edge_weight=pw, P=P, P_abs=P_abs)
