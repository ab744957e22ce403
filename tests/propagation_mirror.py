# coding=utf-8
"""Differentiable torch restatement (CPU, dtype as an argument) of the seven propagation convolutions — what the reference's
nn/conv/{gin,sgc,tagcn,appnp,ssgc,chebynet,le_conv}.py compute, with gcn.py:32-130 (gcn_norm_adj) and
utils/graph_utils.py:554-603 (get_laplacian) underneath — written in the LITERAL order of the reference:

  * a dense [n, n] adjacency built with index_put_(accumulate=True): duplicate edges sum;
  * the GEMM where the reference has it (SGC: first; TAGCN: after the concat; ChebyNet: one per T_i) — no Horner, no Clenshaw,
    no commuted GEMM;
  * self-loops as the reference treats them: gcn_norm_adj ADDS fill * I on top of loops already present (before the degrees
    with renorm, after the scaling without), ChebyNet removes loops first and appends a unit one, le_conv indexes both
    gathered terms by `col`.

Everything is differentiable in x, every kernel and bias, GIN's eps and edge_weight (through the normalisation too).
tests/test_propagation_mirror.py pins the float64 mirror to the reference's own outputs; tests/test_gpu_propagation_backward.py
differentiates it.

`order="rewritten"` evaluates the SAME function in the association the product uses on its narrow-side branches (SGC: hops
first; TAGCN: Horner; ChebyNet: Clenshaw).  It exists for ONE purpose: run in float32, it measures what a float32 evaluation in
that order loses, for the tolerance of the GPU test.  The float64 reference is always `order="literal"`.

`tap`, when a dict, receives "pre" (the pre-activation of the output, when it has an activation) and "hidden" (a list of the
hidden ReLUs' pre-activations): the ReLU-kink rules of the GPU test read them from the float64 run."""
import numpy as np
import torch


def _t(v, dtype):
    if v is None or isinstance(v, torch.Tensor):
        return v
    return torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dtype)


def _index(edge_index):
    ei = edge_index.detach().cpu().numpy() if isinstance(edge_index, torch.Tensor) else np.asarray(edge_index)
    ei = torch.as_tensor(ei.astype(np.int64))
    return ei[0], ei[1]


def dense_adj(edge_index, edge_weight, n, dtype):
    """A[r, c] = sum of the weights of the edges (r, c); ones when edge_weight is None."""
    row, col = _index(edge_index)
    w = torch.ones(row.numel(), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)
    return torch.zeros((n, n), dtype=dtype).index_put_((row, col), w, accumulate=True)


def _zero_where_not_finite(deg, power):
    """deg ** power with inf / nan replaced by 0 (gcn.py:23-29), written so that the gradient at deg == 0 is 0, not nan."""
    ok = deg > 0
    safe = torch.where(ok, deg, torch.ones_like(deg))
    return torch.where(ok, safe ** power, torch.zeros_like(deg))


def gcn_norm_dense(edge_index, edge_weight, n, dtype, renorm=True, improved=False):
    """gcn_norm_adj(norm="both", add_self_loop=True, sym=True) as a dense matrix (gcn.py:62-98)."""
    fill = 2.0 if improved else 1.0
    A = dense_adj(edge_index, edge_weight, n, dtype)
    eye = torch.eye(n, dtype=dtype)
    if renorm:
        A = A + fill * eye                                             # :76-77, on top of loops already present
    dis = _zero_where_not_finite(A.sum(1), -0.5)                       # :80-86
    A = dis[:, None] * A * dis[None, :]                                # :94
    if not renorm:
        A = A + fill * eye                                             # :97-98
    return A


def chebynet_laplacian_dense(edge_index, edge_weight, n, dtype, normalization_type="sym", use_dynamic_lambda_max=False):
    """chebynet_norm_edge (chebynet.py:39-62): loops removed, get_laplacian (graph_utils.py:554-603), times 2 / lambda_max."""
    if normalization_type not in (None, "sym", "rw"):
        raise AssertionError(normalization_type)
    row, col = _index(edge_index)
    w = torch.ones(row.numel(), dtype=dtype) if edge_weight is None else _t(edge_weight, dtype)
    keep = row != col
    row, col, w = row[keep], col[keep], w[keep]
    A = torch.zeros((n, n), dtype=dtype).index_put_((row, col), w, accumulate=True)
    deg = A.sum(1)
    eye = torch.eye(n, dtype=dtype)
    if normalization_type == "sym":
        dis = _zero_where_not_finite(deg, -0.5)
        lap = dis[:, None] * A * dis[None, :] + eye
    elif normalization_type == "rw":
        lap = _zero_where_not_finite(deg, -1.0)[:, None] * A + eye
    else:
        # every stored edge (r, c) carries deg_r - w_e, the appended unit loop deg_r - 1 (:561-569): duplicates sum
        count = torch.zeros((n, n), dtype=dtype).index_put_((row, col), torch.ones_like(w), accumulate=True)
        lap = count * deg[:, None] - A + torch.diag(deg - 1.0)
    lambda_max = 2.0
    if use_dynamic_lambda_max:
        lambda_max = laplacian_lambda_max(edge_index, edge_weight, n, normalization_type)
    return lap * (2.0 / lambda_max)


def laplacian_lambda_max(edge_index, edge_weight, n, normalization_type):
    """Largest-magnitude eigenvalue of the unscaled float64 Laplacian, a constant (LaplacianMaxEigenvalue,
    graph_utils.py:884-909).  'rw' has the spectrum of 'sym' (similar matrices), whose matrix is solved instead."""
    nt = "sym" if normalization_type == "rw" else normalization_type
    ew = edge_weight.detach() if isinstance(edge_weight, torch.Tensor) else edge_weight
    lap = chebynet_laplacian_dense(edge_index, ew, n, torch.float64, nt).numpy()      # scale 2 / 2 = 1
    ev = np.linalg.eigvals(lap)
    return float(ev[np.argmax(np.abs(ev))].real)


def _finish(h, bias, activation, tap):
    if bias is not None:
        h = h + bias
    if activation is None:
        return h
    if activation != "relu":
        raise ValueError(activation)
    if tap is not None:
        tap["pre"] = h
    return torch.relu(h)


def _hidden_relu(h, tap):
    if tap is not None:
        tap.setdefault("hidden", []).append(h)
    return torch.relu(h)


def _mlp(x, kernels, biases, tap):
    """The APPNP / SSGC encoder (appnp.py:60-80): dense layers, ReLU after every one but the last; inference (no dropout)."""
    h = x
    if kernels is not None:
        for i, (k, b) in enumerate(zip(kernels, biases)):
            h = h @ k
            if b is not None:
                h = h + b
            if i < len(kernels) - 1:
                h = _hidden_relu(h, tap)
    return h


def sgc(x, edge_index, edge_weight, k, kernel, bias=None, activation=None, renorm=True, improved=False,
        dtype=torch.float64, order="literal", tap=None):
    x, kernel, bias = _t(x, dtype), _t(kernel, dtype), _t(bias, dtype)
    A = gcn_norm_dense(edge_index, edge_weight, int(x.shape[0]), dtype, renorm, improved)
    if order == "rewritten":
        h = x
        for _ in range(k):
            h = A @ h
        return _finish(h @ kernel, bias, activation, tap)
    h = x @ kernel                                                     # sgc.py:33-36
    for _ in range(k):
        h = A @ h                                                      # :38-39
    return _finish(h, bias, activation, tap)


def tagcn(x, edge_index, edge_weight, k, kernel, bias=None, activation=None, renorm=False, improved=False,
          dtype=torch.float64, order="literal", tap=None):
    x, kernel, bias = _t(x, dtype), _t(kernel, dtype), _t(bias, dtype)
    A = gcn_norm_dense(edge_index, edge_weight, int(x.shape[0]), dtype, renorm, improved)
    F = int(x.shape[1])
    if order == "rewritten":
        ys = [x @ kernel[i * F:(i + 1) * F] for i in range(k + 1)]
        acc = ys[k]
        for i in range(k - 1, -1, -1):
            acc = ys[i] + A @ acc
        return _finish(acc, bias, activation, tap)
    xs = [x]
    for _ in range(k):
        xs.append(A @ xs[-1])                                          # tagcn.py:37-40
    return _finish(torch.cat(xs, dim=-1) @ kernel, bias, activation, tap)      # :42-49


def appnp(x, edge_index, edge_weight, kernels, biases, activation=None, k=10, alpha=0.1, dtype=torch.float64,
          order="literal", tap=None):
    x = _t(x, dtype)
    kernels = None if kernels is None else [_t(v, dtype) for v in kernels]
    biases = None if biases is None else [_t(v, dtype) for v in biases]
    A = gcn_norm_dense(edge_index, edge_weight, int(x.shape[0]), dtype)
    h = _mlp(x, kernels, biases, tap)
    out = h
    for _ in range(k):
        out = A @ out                                                  # appnp.py:84-86
        out = out * (1.0 - alpha) + h * alpha
    return _finish(out, None, activation, tap)


def ssgc(x, edge_index, edge_weight, kernels=None, biases=None, k=10, alpha=0.1, activation=None, dtype=torch.float64,
         order="literal", tap=None):
    x = _t(x, dtype)
    kernels = None if kernels is None else [_t(v, dtype) for v in kernels]
    biases = None if biases is None else [_t(v, dtype) for v in biases]
    A = gcn_norm_dense(edge_index, edge_weight, int(x.shape[0]), dtype)
    h = _mlp(x, kernels, biases, tap)
    out = h * alpha                                                    # ssgc.py:90
    for _ in range(k):
        h = A @ h                                                      # :92-94
        out = out + (1 - alpha) * h / k
    return _finish(out, None, activation, tap)


def chebynet(x, edge_index, edge_weight, k, kernels, bias=None, activation=None, normalization_type="sym",
             use_dynamic_lambda_max=False, dtype=torch.float64, order="literal", tap=None):
    x, bias = _t(x, dtype), _t(bias, dtype)
    kernels = [_t(v, dtype) for v in kernels]
    Lt = chebynet_laplacian_dense(edge_index, edge_weight, int(x.shape[0]), dtype, normalization_type, use_dynamic_lambda_max)
    if order == "rewritten" and k >= 2:
        ys = [x @ kernels[i] for i in range(k)]
        b2, b1 = torch.zeros_like(ys[0]), ys[k - 1]
        for j in range(k - 2, 0, -1):
            b1, b2 = ys[j] + 2.0 * (Lt @ b1) - b2, b1
        return _finish(ys[0] + Lt @ b1 - b2, bias, activation, tap)
    T0 = x
    out = T0 @ kernels[0]                                              # chebynet.py:98-103
    if k > 1:
        T1 = Lt @ x                                                    # :112
        out = out + T1 @ kernels[1]
    for i in range(2, k):
        T2 = Lt @ T1 * 2.0 - T0                                        # :125
        out = out + T2 @ kernels[i]
        T0, T1 = T1, T2
    return _finish(out, bias, activation, tap)


def gin(x, edge_index, mlp_model, eps=0.0, dtype=torch.float64, order="literal", tap=None):
    """mlp_model: a callable of this mirror's dtype (its hidden ReLUs report to `tap` themselves)."""
    x = _t(x, dtype)
    A = dense_adj(edge_index, None, int(x.shape[0]), dtype)           # gin.py:32-34: unweighted
    h = x * (1.0 + eps) + A @ x                                        # :35
    return mlp_model(h)


def le_conv(x, edge_index, edge_weight, self_kernel, self_bias, aggr_self_kernel, aggr_self_bias, aggr_neighbor_kernel,
            aggr_neighbor_bias, activation=None, dtype=torch.float64, order="literal", tap=None):
    x = _t(x, dtype)

    def lin(kernel, bias):
        h = x @ _t(kernel, dtype)
        return h if bias is None else h + _t(bias, dtype)

    A = dense_adj(edge_index, edge_weight, int(x.shape[0]), dtype)
    self_h = lin(self_kernel, self_bias)
    # le_conv.py:40-41: both gathered terms are indexed by `col` -> sum_e w_e (aggr_self_h - aggr_neighbor_h)[col_e]
    diff = lin(aggr_self_kernel, aggr_self_bias) - lin(aggr_neighbor_kernel, aggr_neighbor_bias)
    return _finish(self_h + A @ diff, None, activation, tap)


def structured_graph(seed=1):
    """The one small directed graph of tests/test_gpu_propagation_backward.py: 130 nodes, ~900 edges, weights in [0.5, 1.5];
    explicit self-loops, 50 duplicated edges (with their own weights), rows 127 and 128 without in-edges (they are sources
    only), node 129 without any edge, and hub node 5 with in- and out-degree >= 45 (the transposed plan is skewed too)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, hub = 130, 5
    row = rng.integers(0, 127, size=750)
    col = rng.integers(0, 129, size=750)
    others = np.array([i for i in range(127) if i != hub])
    hub_in, hub_out = rng.permutation(others)[:45], rng.permutation(others)[:45]
    loops = rng.permutation(127)[:8]
    row = np.concatenate([row, np.full(45, hub), hub_out, loops])
    col = np.concatenate([col, hub_in, np.full(45, hub), loops])
    dup = rng.permutation(row.size)[:50]
    row, col = np.concatenate([row, row[dup]]), np.concatenate([col, col[dup]])
    p = rng.permutation(row.size)
    ei = np.stack([row[p], col[p]]).astype(np.int32)
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]).astype(np.float32)
    return dict(n=n, f=14, ei=ei, w=w, hub=hub)
