# coding=utf-8
"""Writes tests/golden/lstm_sage_cases.npz: the outputs of the reference's OWN lstm_graph_sage (nn/conv/graph_sage.py:290),
imported unmodified through oracle/ref_harness.  The function takes the LSTM as an argument, so a numpy float64 LSTM with
Keras's semantics (gates i, f, c, o, zero initial state, return_sequences) is passed where the reference's layer passes
tf.keras.layers.LSTM.  Inputs and weights are stored next to the outputs (``<case>::<name>``).

Every case has a node of degree 0, a node of degree T, repeated neighbours and edges in shuffled order; the cases differ in
concat / normalize / activation / bias and in the number of units.

    python tests/golden/make_lstm_sage_golden.py          # regenerate (needs the reference checkout)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_harness import load_reference   # noqa: E402

OUT = os.path.join(HERE, "lstm_sage_cases.npz")


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


class NumpyLSTM(object):
    def __init__(self, kernel, recurrent_kernel, bias):
        self.kernel, self.recurrent_kernel, self.bias = kernel, recurrent_kernel, bias

    def __call__(self, seq, training=False):
        seq = np.asarray(seq, dtype=np.float64)
        n, T, _ = seq.shape
        U = self.recurrent_kernel.shape[0]
        h = np.zeros((n, U))
        c = np.zeros((n, U))
        out = np.zeros((n, T, U))
        for t in range(T):
            z = seq[:, t] @ self.kernel + h @ self.recurrent_kernel + self.bias
            i, f, g, o = _sigmoid(z[:, :U]), _sigmoid(z[:, U:2 * U]), np.tanh(z[:, 2 * U:3 * U]), _sigmoid(z[:, 3 * U:])
            c = f * c + i * g
            h = o * np.tanh(c)
            out[:, t] = h
        return out


def graph(rng, n):
    """Node 0 has no edge; node 1 has the largest degree (T = 5) with a neighbour repeated; the list is shuffled."""
    rows = [1, 1, 1, 1, 1, 2, 3, 3, 3, n - 1, n - 1, 4, 5, 5]
    cols = [n - 1, 3, 3, 0, 3, 2, n - 1, 0, 0, n - 1, 1, 6, 2, 2]
    ei = np.array([rows, cols], dtype=np.int32)
    return ei[:, rng.permutation(ei.shape[1])]


def cases():
    rng = np.random.Generator(np.random.PCG64(290356))
    out = {}
    for name, U, F, concat, normalize, act, use_bias in [("concat", 6, 5, True, False, "relu", True),
                                                         ("add", 6, 5, False, False, None, True),
                                                         ("concat_normalize", 16, 3, True, True, None, False),
                                                         ("add_normalize", 5, 1, False, True, "relu", True)]:
        n = 9
        out[name] = dict(
            x=rng.normal(size=(n, F)), edge_index=graph(rng, n),
            kernel=rng.normal(size=(F, 4 * U)) * 0.5, recurrent_kernel=rng.normal(size=(U, 4 * U)) * 0.4,
            lstm_bias=rng.normal(size=4 * U) * 0.3, self_kernel=rng.normal(size=(F, U)) * 0.5,
            neighbor_kernel=rng.normal(size=(U, U)) * 0.5,
            bias=(rng.normal(size=2 * U if concat else U) * 0.2) if use_bias else None,
            concat=concat, normalize=normalize, activation=act)
    return out


def run_reference():
    tfg, tf, tfs, backend = load_reference()
    from tf_geometric.nn.conv.graph_sage import lstm_graph_sage
    blob = {"__backend__": np.array(backend), "__cases__": np.array(sorted(cases()))}
    for name, c in cases().items():
        lstm = NumpyLSTM(c["kernel"], c["recurrent_kernel"], c["lstm_bias"])
        act = (lambda v: np.maximum(np.asarray(v), 0.0)) if c["activation"] == "relu" else None
        y = lstm_graph_sage(tf.constant(c["x"]) if hasattr(tf, "constant") else c["x"], c["edge_index"], lstm, c["self_kernel"],
                            c["neighbor_kernel"], bias=c["bias"], activation=act, concat=c["concat"], normalize=c["normalize"])
        for k, v in c.items():
            if v is None:
                continue
            blob["{}::{}".format(name, k)] = np.asarray(v)
        blob["{}::output".format(name)] = np.asarray(y, dtype=np.float64)
    return blob


if __name__ == "__main__":
    blob = run_reference()
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
