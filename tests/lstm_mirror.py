# coding=utf-8
"""A torch mirror of lstm_graph_sage (reference nn/conv/graph_sage.py:290-356 with a Keras-default LSTM) in the dtype of its
inputs: float64 it is the exact reference of the GPU tests (and differentiable, so float64 autograd gives the reference
gradients); float32 on the CPU it is the independent f32 evaluation the GPU tolerance is derived from.

Semantics: node i's sequence is x[col] of its edges in the caller's order (stable sort by row), then zero rows up to
T = max degree; the LSTM (gates i, f, c, o; h_0 = c_0 = 0) is not masked; reduced_h = mean of h_t over all T steps; no edges
-> a zero neighbour term."""
import torch


def neighbor_matrix(edge_index, n_dst, T=None):
    """int64 [n_dst, T]: the source of step t of row i, -1 at pad steps (rows keep the caller's edge order)."""
    ei = torch.as_tensor(edge_index).long().reshape(2, -1).cpu()
    row, col = ei[0], ei[1]
    order = torch.sort(row, stable=True).indices
    row, col = row[order], col[order]
    deg = torch.bincount(row, minlength=n_dst)[:n_dst] if row.numel() else torch.zeros(n_dst, dtype=torch.long)
    if T is None:
        T = int(deg.max()) if deg.numel() and row.numel() else 0
    start = torch.cumsum(deg, 0) - deg
    pos = torch.arange(row.numel()) - start[row]
    nbr = torch.full((n_dst, T), -1, dtype=torch.long)
    keep = pos < T
    nbr[row[keep], pos[keep]] = col[keep]
    return nbr


def aggregate_mirror(P, p_pad, R, nbr):
    """mean over the T steps of h_t; step input = P[nbr] or p_pad where nbr < 0.  [n_dst, U]."""
    n_dst, T = nbr.shape
    U = R.shape[0]
    h = torch.zeros((n_dst, U), dtype=P.dtype)
    c = torch.zeros_like(h)
    total = torch.zeros_like(h)
    for t in range(T):
        idx = nbr[:, t]
        zin = torch.where((idx >= 0).unsqueeze(1), P[idx.clamp(min=0)], p_pad.unsqueeze(0).expand(n_dst, -1))
        z = zin + h @ R
        i, f, g, o = torch.sigmoid(z[:, :U]), torch.sigmoid(z[:, U:2 * U]), torch.tanh(z[:, 2 * U:3 * U]), torch.sigmoid(z[:, 3 * U:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        total = total + h
    return total / T if T > 0 else total


def lstm_sage_mirror(x, edge_index, kernel, recurrent_kernel, lstm_bias, self_kernel, neighbor_kernel, bias=None,
                     activation=None, concat=True, normalize=False, n_dst=None):
    """activation: None or "relu".  n_dst < x.shape[0]: a bipartite plan, the self term is x[:n_dst]."""
    n_dst = x.shape[0] if n_dst is None else n_dst
    nbr = neighbor_matrix(edge_index, n_dst)
    P = x @ kernel + lstm_bias
    reduced = aggregate_mirror(P, lstm_bias, recurrent_kernel, nbr)
    a, b = x[:n_dst] @ self_kernel, reduced @ neighbor_kernel
    out = torch.cat([a, b], dim=1) if concat else a + b
    if bias is not None:
        out = out + bias
    if activation == "relu":
        out = torch.relu(out)
    elif activation is not None:
        raise ValueError(activation)
    if normalize:
        out = out * torch.rsqrt(torch.clamp((out * out).sum(-1, keepdim=True), min=1e-12))
    return out
