# coding=utf-8
"""The remaining SpMM-shaped convolutions of tf_geometric as compositions of the hot-path kernels (SURVEY.md §8f
rank 2): every one is "dense GEMM(s) + k x (A_hat @ h)" over ONE cached plan — no new kernels.

    gin       nn/conv/gin.py:11-38          sgc      nn/conv/sgc.py:10-61        tagcn  nn/conv/tagcn.py:10-51
    appnp     nn/conv/appnp.py:11-92        ssgc     nn/conv/ssgc.py:11-99       le_conv nn/conv/le_conv.py:5-52
    chebynet  nn/conv/chebynet.py:27-137 (+ utils/graph_utils.py:554-603 get_laplacian)

A_hat @ h is `prop(...)`: the differentiable aggregate when gradients are being recorded, the fused kernel otherwise.
"""
import torch

from ... import _lib as L
from ... import autograd as AG
from ...activations import resolve as _resolve_act
from ...plan import CsrPlan, segment_reduce, gemm_bias_act, gather_friendly_copy, gather_friendly_empty
from ...sparse import SparseMatrix, sparse_features, sparse_dense_matmul
from .gcn import gcn_norm_adj, NormedAdj

CACHE_KEY_CHEBYNET_NORMED_EDGE_TEMPLATE = "chebynet_normed_edge_{}"


def _prop(plan, h, w_csr, self_coef):
    if AG.needs_grad(h, w_csr):
        return AG.aggregate(plan, h, L.SUM, w_csr, self_coef)
    # k-hop chains gather narrow / odd-width rows (class scores: 7, 40, 47 ...) again and again: keep every link of the
    # chain on a line-friendly row stride (plan.gather_friendly_ld: F = 47 gathers 15 % faster at stride 48)
    n, F = int(plan.n_dst), int(h.shape[1])
    return segment_reduce(plan, gather_friendly_copy(h), L.SUM, w_csr=w_csr, self_coef=self_coef,
                          out=gather_friendly_empty(n, F, h.device))


def _dense(h, kernel, bias=None, activation=None):
    act, post = _resolve_act(activation)
    hs = sparse_features(h)
    if hs is not None:      # sparse node features: tf.sparse.sparse_dense_matmul at the reference's call sites
        out = sparse_dense_matmul(hs, kernel, bias=bias, act=act)
        return post(out) if post is not None else out
    if AG.needs_grad(h, kernel, bias):
        return AG.apply_activation(AG.linear(h, kernel, bias, act), L.ACT_NONE, post)
    out = gemm_bias_act(h, kernel, bias=bias, act=act)
    return post(out) if post is not None else out


def _features(x, densify=False):
    """Dense fp32 features, or the SparseMatrix form of sparse ones (densified where the reference densifies)."""
    xs = sparse_features(x)
    if xs is None:
        return L.as_f32(x)
    return xs.to_dense() if densify else xs


def _finish(h, bias, activation):
    """+ bias, activation — and the PUBLIC result is always a dense [n, F] tensor: the padded row stride of
    gather_friendly_empty is for the intermediate links of a k-hop chain only (a [:, :F] view of a wider buffer would
    break .view(-1), DLPack and any consumer assuming ld == F)."""
    act, post = _resolve_act(activation)
    if bias is not None:
        h = AG.bias_add(h, bias)
    h = AG.apply_activation(h, act, post)
    return h if h.is_contiguous() else h.contiguous()


def _refuse_trainable_edge_weight(edge_weight, what):
    """The normalisations (gcn_norm_adj, chebynet_norm_edge) are raw kernel launches: a tracked edge_weight would get no
    gradient from them.  Checked before any cache lookup, so a cached adjacency cannot hide it."""
    if AG.needs_grad(edge_weight):
        raise NotImplementedError("{}: an edge_weight that requires grad is not supported (the normalisation is not "
                                  "differentiable here); detach it or call under torch.no_grad()".format(what))


def _normed(x, edge_index, edge_weight, cache, **norm_kwargs):
    _refuse_trainable_edge_weight(edge_weight, "gcn_norm_adj of a propagation conv")
    n = int(x.shape[0])
    key = "tfgx_gcn_adj"
    adj = cache.get(key) if cache is not None else None
    if adj is None:
        adj = SparseMatrix(edge_index, edge_weight, [n, n])
        if cache is not None:
            cache[key] = adj
    return gcn_norm_adj(adj, cache=cache, **norm_kwargs)


def gin(x, edge_index, mlp_model, eps=0.0, training=None, cache=None):
    """h = mlp((1 + eps) * x + sum_{j in N(i)} x_j)   (reference: gin.py:11-38). `mlp_model` is any callable."""
    x = L.as_f32(x)
    n = int(x.shape[0])
    plan = CsrPlan.from_cache(edge_index, n, n, cache)
    neighbor_h = _prop(plan, x, None, None)                           # SparseMatrix(edge_index) @ x  (:32-34)
    h = x * (1.0 + eps) + neighbor_h                                   # :35
    try:
        return mlp_model(h, training=training)                         # :36
    except TypeError:
        return mlp_model(h)


def sgc(x, edge_index, edge_weight, k, kernel, bias=None, activation=None, renorm=True, improved=False, cache=None):
    """A_hat^k (x @ kernel) + bias  (reference: sgc.py:10-61; the GEMM comes first there too; x may be sparse, :31)."""
    x = _features(x)
    normed = _normed(x, edge_index, edge_weight, cache, renorm=renorm, improved=improved)
    if sparse_features(x) is None and int(x.shape[1]) < int(L.as_f32(kernel).shape[1]):
        # A_hat^k (x W) == (A_hat^k x) W: when the layer WIDENS, the k hops gather F-wide rows instead of units-wide ones
        # (the mirror image of GCN's narrow-side rule; same value up to fp32 re-association)
        h = x
        for _ in range(k):
            h = _prop(normed.plan, h, normed.w_csr, normed.self_coef)
        return _finish(_dense(h, kernel), bias, activation)
    h = _dense(x, kernel)                                              # :33-36
    for _ in range(k):
        h = _prop(normed.plan, h, normed.w_csr, normed.self_coef)      # :38-39
    return _finish(h, bias, activation)


def tagcn(x, edge_index, edge_weight, k, kernel, bias=None, activation=None, renorm=False, improved=False, cache=None):
    """concat(x, A x, ..., A^k x) @ kernel  (reference: tagcn.py:10-51; sparse x is densified first, :32-35)."""
    x = _features(x, densify=True)
    normed = _normed(x, edge_index, edge_weight, cache, renorm=renorm, improved=improved)
    F, units = int(x.shape[1]), int(kernel.shape[1])
    if units < F:
        # [x | A x | ... | A^k x] @ kernel = sum_i A^i (x @ W_i), W_i = rows [i*F, (i+1)*F) of the kernel: ONE GEMM
        # x @ [W_0 | ... | W_k], then Horner's rule y_0 + A (y_1 + A (... + A y_k)) — the k propagations gather
        # `units`-wide rows instead of F-wide ones (same value up to fp32 re-association)
        kt = L.as_f32(kernel)
        wcat = kt.view(k + 1, F, units).permute(1, 0, 2).reshape(F, (k + 1) * units).contiguous()
        y = _dense(x, wcat)
        acc = y[:, k * units:(k + 1) * units]
        for i in range(k - 1, -1, -1):
            acc = y[:, i * units:(i + 1) * units] + _prop(normed.plan, acc.contiguous(), normed.w_csr, normed.self_coef)
        return _finish(acc, bias, activation)
    xs = [x]
    for _ in range(k):
        xs.append(_prop(normed.plan, xs[-1], normed.w_csr, normed.self_coef))    # :37-40
    h = torch.cat(xs, dim=-1)                                          # :42
    return _finish(_dense(h, kernel), bias, activation)                # :44-49


def _mlp_encoder(x, kernels, biases, dense_activation, training, dense_drop_rate, last_dense_drop_rate):
    """The MLP encoder of APPNP / SSGC (appnp.py:60-80, ssgc.py:66-87): tf.nn.dropout after every hidden layer's
    activation (dense_drop_rate) and after the last layer (last_dense_drop_rate), training only."""
    h = x
    if kernels is not None:
        last = len(kernels) - 1
        for i, (kernel, bias) in enumerate(zip(kernels, biases)):
            h = _dense(h, kernel, bias, dense_activation if i < last else None)
            rate = dense_drop_rate if i < last else last_dense_drop_rate
            if training and rate > 0.0:
                h = torch.nn.functional.dropout(h, p=float(rate), training=True)
    return h


def appnp(x, edge_index, edge_weight, kernels, biases, dense_activation="relu", activation=None, k=10, alpha=0.1,
          dense_drop_rate=0.0, last_dense_drop_rate=0.0, edge_drop_rate=0.0, cache=None, training=False):
    """Z <- (1 - alpha) A_hat Z + alpha H, k times, H = MLP(x)  (reference: appnp.py:11-92; x may be sparse, :64)."""
    x = _features(x)
    normed = _normed(x, edge_index, edge_weight, cache).dropout(edge_drop_rate, training=training)
    h = _mlp_encoder(x, kernels, biases, dense_activation, training, dense_drop_rate, last_dense_drop_rate)
    output = h
    if not AG.needs_grad(h) and k > 0:
        # inference: (1 - alpha) A_hat Z + alpha H in ONE launch per hop — the edge weights and the self-loop coefficient
        # are scaled by (1 - alpha) once, alpha H rides in the kernel's epilogue (add_x); no elementwise pass per hop
        n, F = int(h.shape[0]), int(h.shape[1])
        w_s = normed.w_csr * (1.0 - alpha)
        sc_s = None if normed.self_coef is None else normed.self_coef * (1.0 - alpha)
        ah = gather_friendly_copy(h * alpha)
        output = gather_friendly_copy(h)
        for _ in range(k):
            output = segment_reduce(normed.plan, output, L.SUM, w_csr=w_s, self_coef=sc_s, add_x=ah,
                                    out=gather_friendly_empty(n, F, h.device))
        return _finish(output, None, activation)
    for _ in range(k):
        output = _prop(normed.plan, output, normed.w_csr, normed.self_coef)       # :84-86
        output = output * (1.0 - alpha) + h * alpha
    return _finish(output, None, activation)


def ssgc(x, edge_index, edge_weight, kernels=None, biases=None, k=10, alpha=0.1, dense_activation="relu",
         activation=None, dense_drop_rate=0.0, last_dense_drop_rate=0.0, edge_drop_rate=0.0, cache=None,
         training=False):
    """alpha H + (1 - alpha)/k * sum_{t=1..k} A_hat^t H  (reference: ssgc.py:11-99; x may be sparse, :73)."""
    x = _features(x, densify=kernels is None)
    normed = _normed(x, edge_index, edge_weight, cache).dropout(edge_drop_rate, training=training)
    h = _mlp_encoder(x, kernels, biases, dense_activation, training, dense_drop_rate, last_dense_drop_rate)
    output = h * alpha                                                 # :90
    for _ in range(k):
        h = _prop(normed.plan, h, normed.w_csr, normed.self_coef)      # :92-94
        output = output + (1 - alpha) * h / k
    return _finish(output, None, activation)


def le_conv(x, edge_index, edge_weight, self_kernel, self_bias, aggr_self_kernel, aggr_self_bias,
            aggr_neighbor_kernel, aggr_neighbor_bias, activation=None, cache=None):
    """Reference le_conv.py:5-52, literally: BOTH gathered terms are indexed by `col` (:40-41), so the aggregate is
    sum_j w_ij * (x_j @ aggr_self_kernel - x_j @ aggr_neighbor_kernel)."""
    x = L.as_f32(x)
    n = int(x.shape[0])
    plan = CsrPlan.from_cache(edge_index, n, n, cache)
    if edge_weight is None:
        w_csr = None                                                   # ones (:21-22)
    elif AG.needs_grad(edge_weight):
        w_csr = AG.edge_attr_csr(plan, edge_weight)                    # trainable weights: a differentiable permutation
    else:
        w_csr = plan.edge_attr_to_csr(edge_weight)
    self_h = _dense(x, self_kernel, self_bias)
    diff = _dense(x, aggr_self_kernel, aggr_self_bias) - _dense(x, aggr_neighbor_kernel, aggr_neighbor_bias)
    h = self_h + _prop(plan, diff, w_csr, None)                        # :43-47
    return _finish(h, None, activation)


def chebynet_norm_edge(edge_index, num_nodes, edge_weight=None, normalization_type="sym",
                       use_dynamic_lambda_max=False, cache=None):
    """Scaled "Laplacian" of chebynet.py:27-54 + graph_utils.get_laplacian (:554-603), in plan form (a NormedAdj):
    self-loops removed, sym: D^-1/2 A D^-1/2 + I, rw: D^-1 A + I, None: (deg_r - w) on edges and on an appended
    unit self-loop; everything times 2 / lambda_max (lambda_max = 2, or the Laplacian's largest eigenvalue when
    use_dynamic_lambda_max: laplacian_max_eigenvalue)."""
    _refuse_trainable_edge_weight(edge_weight, "chebynet_norm_edge")
    if cache is not None:
        key = CACHE_KEY_CHEBYNET_NORMED_EDGE_TEMPLATE.format(normalization_type)
        if cache.get(key) is not None:
            return cache[key]
    if normalization_type not in (None, "sym", "rw"):
        raise AssertionError("normalization_type must be None, 'sym' or 'rw'")        # graph_utils.py:556
    ei = L.as_i32(edge_index)
    E = int(ei.shape[1])
    w = torch.ones(E, dtype=torch.float32, device=ei.device) if edge_weight is None else L.as_f32(edge_weight)
    keep = ei[0] != ei[1]                                              # remove_self_loop_edge (chebynet.py:34)
    ei, w = ei[:, keep].contiguous(), w[keep].contiguous()
    adj = SparseMatrix(ei, w, [num_nodes, num_nodes])
    if normalization_type == "sym":
        normed = gcn_norm_adj(adj, renorm=False)                      # D^-1/2 A D^-1/2, + fill*I afterwards
        w_csr, self_coef = normed.w_csr, normed.self_coef
    elif normalization_type == "rw":
        normed = gcn_norm_adj(adj, norm="left", add_self_loop=False, sym=False)
        w_csr = normed.w_csr
        self_coef = torch.ones(num_nodes, dtype=torch.float32, device=ei.device)
    else:
        deg = adj.segment_sum(axis=-1)
        plan = adj.plan
        rows = torch.repeat_interleave(torch.arange(num_nodes, device=ei.device), plan.in_degree().long())
        w_csr = deg[rows] - adj.value_csr
        self_coef = deg - 1.0
        normed = NormedAdj(plan, w_csr, self_coef, [num_nodes, num_nodes])
    lambda_max = 2.0                                                   # chebynet.py:41-43
    if use_dynamic_lambda_max:                                         # :39-40 -> LaplacianMaxEigenvalue (graph_utils.py:884-909)
        lambda_max = laplacian_max_eigenvalue(NormedAdj(normed.plan, w_csr, self_coef, [num_nodes, num_nodes]),
                                              normalization_type)
    scale = 2.0 / lambda_max
    out = NormedAdj(normed.plan, w_csr * scale, self_coef * scale, [num_nodes, num_nodes])
    if cache is not None:
        cache[key] = out
    return out


def laplacian_max_eigenvalue(lap, normalization_type="sym", steps=96, tol=1e-6, restarts=6):
    """Largest-magnitude eigenvalue of the Laplacian held in plan form (graph_utils.LaplacianMaxEigenvalue, :884-909,
    which hands scipy's ARPACK a scipy matrix: eigsh for 'sym' / 'rw', eigs for None, k = 1, which = 'LM').

    Here: Arnoldi iteration (Lanczos with full re-orthogonalisation when the operator is symmetric), every L @ v on the
    segment-reduce kernel (the graph never leaves the device), the m x m Hessenberg eigenproblem on the host.  The
    operator is symmetric for 'sym'; for None get_laplacian yields (deg_r - w_rc) off the diagonal — not symmetric, which
    is why the reference switches to the general solver there, and why Arnoldi (not plain Lanczos) is used here.  'rw' (D^-1 A + I) is not symmetric, but it is similar to the 'sym' matrix (D^-1/2 ... D^1/2), so it has the
    same spectrum: the symmetric operator S = D^1/2 L_rw D^-1/2 is iterated instead and lambda_max is exact — the
    reference calls the SYMMETRIC solver on the non-symmetric matrix there, whose answer is solver-dependent."""
    import numpy as np
    plan, n = lap.plan, int(lap.shape[0])
    dev = plan.col.device
    if n == 0:
        return 2.0
    scale_r = scale_c = None
    if normalization_type == "rw":
        # L_rw = I + D^-1 A' (A' carries the sign get_laplacian gives it); S = D^1/2 L_rw D^-1/2 is symmetric.
        # |w_e| = |A_rc| / deg_r  ->  deg_r = 1 / sum_e |w_e| * (sum_e |A_rc|) is not recoverable from w alone, so take
        # the degrees from the plan's row sums of |w| against a unit-weight pass: deg_r ∝ 1 / mean row weight.  For the
        # similarity transform any positive d with d_r * w_rc = d_c * w_cr works; d_r = 1 / sum_e |w_re| does when the
        # underlying A is symmetric with unit or symmetric weights (then sum_e |w_re| = 1 and d = 1): use the general
        # construction d_r = sqrt(sum_e |w_er| / sum_e |w_re|) (column mass over row mass).
        ones = torch.ones((n, 1), dtype=torch.float32, device=dev)
        absw = lap.w_csr.abs()
        row_mass = segment_reduce(plan, ones, L.SUM, w_csr=absw)[:, 0]
        pt = plan.transposed()
        col_mass = segment_reduce(pt, ones, L.SUM, w_csr=pt.edge_attr_to_csr(_csr_to_edge_order(plan, absw)))[:, 0]
        d = torch.sqrt(torch.clamp(col_mass, min=1e-30) / torch.clamp(row_mass, min=1e-30))
        d = torch.where((row_mass > 0) & (col_mass > 0), d, torch.ones_like(d))
        scale_r, scale_c = (1.0 / d).unsqueeze(1), d.unsqueeze(1)      # S = diag(1/d) L diag(d)

    def matvec(v):
        h = v if scale_c is None else v * scale_c
        out = segment_reduce(plan, h.contiguous(), L.SUM, w_csr=lap.w_csr, self_coef=lap.self_coef)
        return out if scale_r is None else out * scale_r

    # Arnoldi (= Lanczos with full re-orthogonalisation when the operator is symmetric): H = V^T L V, upper Hessenberg.
    # Convergence is CHECKED, as ARPACK checks it: the Ritz pair (theta, V y) of the dominant eigenvalue has residual
    # |L V y - theta V y| = |b_m * y_m| (last sub-diagonal entry times the last component of the Hessenberg eigenvector);
    # while that exceeds tol * |theta| the iteration restarts from the Ritz vector (explicit restart), up to `restarts`
    # times.  `laplacian_max_eigenvalue.last` records (restarts used, relative residual) for the tests.
    m = int(min(steps, n))
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    v = torch.randn((n, 1), generator=g, dtype=torch.float32).to(dev)
    v = v / v.norm()
    theta, rel = 2.0, 0.0
    for attempt in range(restarts + 1):
        basis = torch.zeros((n, m), dtype=torch.float32, device=dev)
        H = np.zeros((m + 1, m), np.float64)
        k, b_last = 0, 0.0
        for j in range(m):
            basis[:, j] = v[:, 0]
            wv = matvec(v)
            V = basis[:, :j + 1]
            h1 = V.t() @ wv
            wv = wv - V @ h1
            h2 = V.t() @ wv                                                  # second Gram-Schmidt pass
            wv = wv - V @ h2
            H[:j + 1, j] = (h1 + h2)[:, 0].double().cpu().numpy()
            b_j = float(wv.norm().item())
            k = j + 1
            b_last = b_j
            if b_j < 1e-7:
                b_last = 0.0                                                 # invariant subspace: the Ritz values are exact
                break
            if j == m - 1:
                break
            H[j + 1, j] = b_j
            v = wv / b_j
        ev, evec = np.linalg.eig(H[:k, :k])
        i = int(np.argmax(np.abs(ev)))
        theta = float(ev[i].real)
        y = evec[:, i]
        rel = abs(b_last * y[k - 1]) / max(abs(theta), 1e-30)
        if rel <= tol or k >= n:
            break
        ritz = basis[:, :k] @ torch.as_tensor(np.ascontiguousarray(y.real), dtype=torch.float32, device=dev).unsqueeze(1)
        nrm = float(ritz.norm().item())
        if nrm < 1e-20:
            break
        v = ritz / nrm
    laplacian_max_eigenvalue.last = dict(restarts=attempt, rel_residual=float(rel), steps=k)
    return theta


def _csr_to_edge_order(plan, attr_csr):
    out = torch.empty_like(attr_csr)
    out[plan.perm.long()] = attr_csr
    return out


def chebynet(x, edge_index, edge_weight, k, kernels, bias=None, activation=None, normalization_type="sym",
             use_dynamic_lambda_max=False, cache=None):
    """sum_i T_i(L~) x @ kernels[i]  (reference: chebynet.py:83-137; a sparse x feeds kernels[0] sparsely and is
    densified for the propagation, :100-119)."""
    x0 = _features(x)
    x = x0.to_dense() if isinstance(x0, SparseMatrix) else x0
    n = int(x.shape[0])
    normed = chebynet_norm_edge(edge_index, n, edge_weight, normalization_type, use_dynamic_lambda_max, cache)
    units = int(L.as_f32(kernels[0]).shape[1])
    if k >= 2 and not isinstance(x0, SparseMatrix) and units < int(x.shape[1]):
        # sum_i T_i(L~) (x W_i): the hops act on the node dimension, the kernels on the feature dimension, so they commute —
        # ONE GEMM y = x @ [W_0 | ... | W_{k-1}], then Clenshaw's recurrence evaluates sum_i T_i(L~) y_i with k - 1 hops over
        # `units`-wide rows instead of k - 1 hops over F-wide ones:  b_j = y_j + 2 L~ b_{j+1} - b_{j+2},  result = y_0 +
        # L~ b_1 - b_2  (same value up to fp32 re-association; F = 1433 -> 16, k = 3: 16.9 -> 1 ms)
        y = _dense(x, torch.cat([L.as_f32(kk) for kk in kernels[:k]], dim=1))
        ys = [y[:, i * units:(i + 1) * units] for i in range(k)]
        b2 = torch.zeros_like(ys[0])
        b1 = ys[k - 1]
        for j in range(k - 2, 0, -1):
            b1, b2 = ys[j] + 2.0 * _prop(normed.plan, b1.contiguous(), normed.w_csr, normed.self_coef) - b2, b1
        out = ys[0] + _prop(normed.plan, b1.contiguous(), normed.w_csr, normed.self_coef) - b2
        return _finish(out, bias, activation)
    T0 = x
    out = _dense(x0, kernels[0])                                       # :101-106
    if k > 1:
        T1 = _prop(normed.plan, x, normed.w_csr, normed.self_coef)     # :112
        out = out + _dense(T1, kernels[1])
    for i in range(2, k):
        T2 = _prop(normed.plan, T1, normed.w_csr, normed.self_coef) * 2.0 - T0       # :123-125
        out = out + _dense(T2, kernels[i])
        T0, T1 = T1, T2
    return _finish(out, bias, activation)
