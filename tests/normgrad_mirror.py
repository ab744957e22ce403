# coding=utf-8
"""The GCN normalisation (nn/conv/gcn.py gcn_norm_adj; reference gcn.py:32-130) twice over, on the CPU:

``restatement``  float64 torch, op for op what the reference computes, differentiable by torch autograd.  The degree powers are
                 the MASKED power ``where(ok, d, 1).pow(e) * ok`` with ok = "d ** e is finite": the forward's value (inf / nan
                 -> 0) and a zero derivative wherever the factor was zeroed — tf.where would hand NaN to the gradient of an
                 isolated node instead.  absolute=True keeps every value and back-propagates |cotangent| through |local
                 Jacobians| (asap_mirror._Ops), which yields the sum of |terms| of every gradient entry.
``closed_form``  numpy, the formulas of include/tfgx_normgrad.h: what the three backward kernels compute.

tests/test_normgrad_mirror.py holds the closed form to autograd on the restatement for every legal configuration;
tests/test_gpu_gcn_norm_backward.py holds the kernels to the restatement."""
import itertools

import numpy as np
import torch

from asap_mirror import _Ops, _seg_sum


def configs():
    """The 24 legal (norm, sym, add_self_loop, renorm, improved): sym and renorm only matter for norm="both"."""
    out = [("both", sym, asl, renorm, imp) for sym, asl, renorm, imp in itertools.product([True, False], repeat=4)]
    for norm in ("left", "right"):
        out += [(norm, True, asl, True, imp) for asl, imp in itertools.product([True, False], repeat=2)]
    return out


def config_id(cfg):
    norm, sym, asl, renorm, imp = cfg
    return "{}-{}-{}-{}-{}".format(norm, "sym" if sym else "nosym", "loop" if asl else "noloop",
                                   "renorm" if renorm else "plain", "improved" if imp else "unit")


class _AbsMaskedPow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, e):
        ok = torch.isfinite(d.pow(e))
        safe = torch.where(ok, d, torch.ones_like(d))
        ctx.save_for_backward(safe, ok)
        ctx.e = e
        return safe.pow(e) * ok

    @staticmethod
    def backward(ctx, g):
        safe, ok = ctx.saved_tensors
        return g.abs() * (ctx.e * safe.pow(ctx.e - 1.0)).abs() * ok, None


def masked_pow(ops, d, e):
    if ops.absolute:
        return _AbsMaskedPow.apply(d, e)
    ok = torch.isfinite(d.detach().pow(e))
    return torch.where(ok, d, torch.ones_like(d)).pow(e) * ok


def restatement(ops, row, col, w, n_rows, n_cols, cfg):
    """(w_out [E], self_coef [n_rows] or None) for raw weights w in the order of (row, col) (int64 tensors)."""
    norm, sym, asl, renorm, improved = cfg
    fill = 2.0 if improved else 1.0
    if norm == "both":
        diag = fill if (asl and renorm) else 0.0
        deg_r = _seg_sum(row, w, n_rows) + diag
        deg_c = deg_r if sym else _seg_sum(col, w, n_cols) + diag
        pr, pc = masked_pow(ops, deg_r, -0.5), masked_pow(ops, deg_c, -0.5)
        w_out = ops.mul(ops.mul(pr[row], w), pc[col])
        if not asl:
            return w_out, None
        return w_out, (ops.mul(pr, pc) * fill if renorm else torch.full((n_rows,), fill, dtype=w.dtype))
    diag = fill if asl else 0.0
    q = masked_pow(ops, _seg_sum(row, w, n_rows) + diag, -1.0)
    w_out = ops.mul(q[row], w) if norm == "left" else ops.mul(w, q[col])
    return w_out, (q * fill if asl else None)


def reference_gradient(row, col, w, n_rows, n_cols, cfg, c, s, absolute=False):
    """d/dw of sum_e c_e w_out_e + sum_v s_v self_coef_v by float64 autograd on the restatement (numpy in, numpy out);
    absolute=True: the sum of |terms| of each entry."""
    ops = _Ops(absolute)
    leaf = torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True)
    tr, tc = torch.from_numpy(np.asarray(row, np.int64)), torch.from_numpy(np.asarray(col, np.int64))
    w_out, sc = restatement(ops, tr, tc, leaf, n_rows, n_cols, cfg)
    ct = lambda a: torch.from_numpy(np.abs(a) if absolute else np.asarray(a, np.float64))     # noqa: E731
    loss = (w_out * ct(c)).sum()
    if sc is not None and sc.requires_grad:
        loss = loss + (sc * ct(s)).sum()
    loss.backward()
    return leaf.grad.numpy()


def _inv_pow(d, half):
    with np.errstate(all="ignore"):
        v = np.power(d, -0.5) if half else 1.0 / d
    return np.where(np.isfinite(v), v, 0.0)


def _inv_pow_grad(d, half):
    f = _inv_pow(d, half)
    with np.errstate(all="ignore"):
        v = -0.5 * f * f * f if half else -(f * f)
    return np.where(np.isfinite(v), v, 0.0)


def closed_form(row, col, w, n_rows, n_cols, cfg, G, S):
    """dL/dw from G = dL/dw_out and S = dL/dself_coef (None: absent), float64 numpy, in the order of (row, col)."""
    norm, sym, asl, renorm, improved = cfg
    fill = 2.0 if improved else 1.0
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    w, G = np.asarray(w, np.float64), np.asarray(G, np.float64)
    seg = lambda idx, v, n: np.bincount(idx, weights=v, minlength=n)[:n] if len(idx) else np.zeros(n)    # noqa: E731
    if norm == "both":
        diag = fill if (asl and renorm) else 0.0
        deg_r = seg(row, w, n_rows) + diag
        deg_c = deg_r if sym else seg(col, w, n_cols) + diag
        p_r, p_c = _inv_pow(deg_r, True), _inv_pow(deg_c, True)
        A = seg(row, G * w * p_c[col], n_rows)
        B = seg(col, G * w * p_r[row], n_cols)
        if asl and renorm and S is not None:
            A = A + S * fill * p_c
            B = B + S * fill * p_r
        if sym:
            D = (A + B) * _inv_pow_grad(deg_r, True)
            return G * p_r[row] * p_c[col] + D[row]
        D_r, D_c = A * _inv_pow_grad(deg_r, True), B * _inv_pow_grad(deg_c, True)
        return G * p_r[row] * p_c[col] + D_r[row] + D_c[col]
    deg_r = seg(row, w, n_rows) + (fill if asl else 0.0)
    q = _inv_pow(deg_r, False)
    if norm == "left":
        T = seg(row, G * w, n_rows)
        if asl and S is not None:
            T = T + S * fill
        return G * q[row] + (T * _inv_pow_grad(deg_r, False))[row]
    T = np.zeros(n_rows)                        # right: columns are node ids below n_cols <= n_rows
    T[:n_cols] = seg(col, G * w, n_cols)
    if asl and S is not None:
        T = T + S * fill
    return G * q[col] + (T * _inv_pow_grad(deg_r, False))[row]


def sweep_graph(negate_row=None):
    """n = 37, 300 random edges with duplicates and some self-loops; node 36 heads no edge (row degree 0), node 35 is no
    edge's column.  Weights U(0.5, 1.5); negate_row: the weights of that row negated (a negative degree)."""
    rng = np.random.Generator(np.random.PCG64(2024))
    n, E = 37, 300
    row = rng.integers(0, 36, E)                 # never 36
    col = rng.integers(0, 36, E)
    col[:6] = row[:6]                            # input self-loops
    row[6:12], col[6:12] = row[12:18], col[12:18]      # duplicates
    col[col == 35] = 36                          # never 35; 36 does appear as a column
    w = rng.uniform(0.5, 1.5, E)
    if negate_row is not None:
        w[row == negate_row] *= -1.0
    c, s = rng.standard_normal(E), rng.standard_normal(n)
    return dict(n=n, row=row.astype(np.int32), col=col.astype(np.int32), w=w.astype(np.float32), c=c, s=s)


def hub_graph():
    """n = 64: node 5 heads 2100 edges (a long row), node 9 is the column of 2100 (a long column), plus 400 random edges."""
    rng = np.random.Generator(np.random.PCG64(77))
    n = 64
    row = np.concatenate([np.full(2100, 5), rng.integers(0, n, 2100), rng.integers(0, n, 400)])
    col = np.concatenate([rng.integers(0, n, 2100), np.full(2100, 9), rng.integers(0, n, 400)])
    order = rng.permutation(len(row))
    row, col = row[order], col[order]
    E = len(row)
    return dict(n=n, row=row.astype(np.int32), col=col.astype(np.int32), w=rng.uniform(0.5, 1.5, E).astype(np.float32),
                c=rng.standard_normal(E), s=rng.standard_normal(n))


def rect_graph(n_rows, n_cols, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    E = 40
    row, col = rng.integers(0, n_rows, E), rng.integers(0, n_cols, E)
    return dict(n_rows=n_rows, n_cols=n_cols, row=row.astype(np.int32), col=col.astype(np.int32),
                w=rng.uniform(0.5, 1.5, E).astype(np.float32), c=rng.standard_normal(E), s=rng.standard_normal(n_rows))


def longest_reduction(row, col, n_rows, n_cols):
    return int(max(np.bincount(row, minlength=n_rows).max(), np.bincount(col, minlength=n_cols).max())) + 2


def gcn_mirror(ops, x, row, col, w, n, cfg, kernel=None, bias=None):
    """nn.gcn on a square graph in float64: A_hat (x @ kernel) + bias with A_hat from the restatement."""
    w_out, sc = restatement(ops, row, col, w, n, n, cfg)
    h = x if kernel is None else ops.mm(x, kernel)
    out = _seg_sum(row, ops.mul(w_out.unsqueeze(1), h[col]), n)
    if sc is not None:
        out = out + ops.mul(sc.unsqueeze(1), h)
    return out if bias is None else out + bias
