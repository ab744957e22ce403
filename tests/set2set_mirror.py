# coding=utf-8
"""A torch mirror of set2set (reference nn/pool/set2set.py:8-42 with a Keras-default LSTM and the segment_softmax of
nn/kernel/segment.py:26-33, epsilon included) in the dtype of its inputs: float64 it is the exact reference of the GPU tests
(and differentiable, so float64 autograd gives the reference gradients); float32 on the CPU it is the independent f32
evaluation the GPU tolerance is derived from.

batch_graphs=False is the reference's literal call: the [G, 2F] query tensor goes through the LSTM as ONE sequence of G
steps with a [1, F] state that is carried from round to round.  batch_graphs=True: G sequences of one step, a [G, F] state."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set2set_cases.npz")


def lstm_mirror(seq, kernel, recurrent_kernel, bias, h0, c0):
    """seq [B, T, Fin], h0 / c0 [B, U] -> (every h_t [B, T, U], last h, last c); gates i, f, c, o."""
    B, T, _ = seq.shape
    U = recurrent_kernel.shape[0]
    h, c = h0.expand(B, U), c0.expand(B, U)
    out = []
    for t in range(T):
        z = seq[:, t] @ kernel + bias + h @ recurrent_kernel
        i, f, g, o = torch.sigmoid(z[:, :U]), torch.sigmoid(z[:, U:2 * U]), torch.tanh(z[:, 2 * U:3 * U]), torch.sigmoid(z[:, 3 * U:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        out.append(h)
    seq_out = torch.stack(out, dim=1) if out else seq.new_zeros((B, 0, U))
    return seq_out, h, c


def attend_mirror(x, ids, q, num_graphs):
    """r [G, F] and the attention weights a [N]: a = exp(e - stop_gradient(max)) / (sum + 1e-8), e_n = <x_n, q_graph(n)>."""
    ids = ids.long()
    e = (x * q[ids]).sum(-1)
    m = torch.full((num_graphs,), float("-inf"), dtype=x.dtype).scatter_reduce(0, ids, e.detach(), "amax", include_self=True)
    p = torch.exp(e - m[ids])
    D = torch.zeros(num_graphs, dtype=x.dtype).index_add(0, ids, p) + 1e-8
    a = p / D[ids]
    r = torch.zeros((num_graphs, x.shape[1]), dtype=x.dtype).index_add(0, ids, x * a.unsqueeze(1))
    return r, a


def set2set_mirror(x, ids, kernel, recurrent_kernel, bias, num_iterations, num_graphs=None, batch_graphs=False):
    ids = torch.as_tensor(ids).long()
    G = int(ids.max()) + 1 if num_graphs is None else int(num_graphs)
    F = x.shape[1]
    h = torch.zeros((G, 2 * F), dtype=x.dtype)
    rows = G if batch_graphs else 1
    state_h, state_c = torch.zeros((rows, F), dtype=x.dtype), torch.zeros((rows, F), dtype=x.dtype)
    for _ in range(num_iterations):
        seq = h.unsqueeze(1) if batch_graphs else h.unsqueeze(0)
        out, state_h, state_c = lstm_mirror(seq, kernel, recurrent_kernel, bias, state_h, state_c)
        q = out.reshape(G, F)
        r, _ = attend_mirror(x, ids, q, G)
        h = torch.cat([q, r], dim=-1)
    return h


# ---- the golden cases (tests/golden/make_set2set_golden.py), shared by the non-GPU and the GPU tests
def golden_cases():
    blob = np.load(GOLDEN)
    out = {}
    for name in blob["__cases__"].tolist():
        c = {k.split("::", 1)[1]: blob[k] for k in blob.files if k.startswith(name + "::")}
        c["num_iterations"] = int(c["num_iterations"])
        out[name] = c
    return out


def mirror_of_case(c, dtype=torch.float64, batch_graphs=False):
    t = lambda k: torch.as_tensor(np.asarray(c[k], dtype=np.float64)).to(dtype)      # noqa: E731
    return set2set_mirror(t("x"), c["node_graph_index"], t("kernel"), t("recurrent_kernel"), t("bias"), c["num_iterations"],
                            batch_graphs=batch_graphs)
