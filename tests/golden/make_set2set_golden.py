# coding=utf-8
"""Writes tests/golden/set2set_cases.npz: the outputs of the reference's OWN set2set (nn/pool/set2set.py:8), imported
unmodified through oracle/ref_harness.  The function takes the LSTM as an argument, so a numpy float64 LSTM with Keras's
semantics (gates i, f, c, o; it honours initial_state and returns (sequence, h, c)) is passed where the reference's layer
passes tf.keras.layers.LSTM(F, return_sequences=True, return_state=True).  Inputs and weights are stored next to the outputs
(``<case>::<name>``).

The cases cover shuffled graph ids, an empty graph in the middle of the batch, a graph of one node, a batch of one graph,
num_iterations 1 / 3 / 4 and F = 1 / 5.

    python tests/golden/make_set2set_golden.py          # regenerate (needs the reference checkout)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_harness import load_reference   # noqa: E402

OUT = os.path.join(HERE, "set2set_cases.npz")


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


class NumpyLSTM(object):
    def __init__(self, kernel, recurrent_kernel, bias):
        self.kernel, self.recurrent_kernel, self.bias = kernel, recurrent_kernel, bias

    def __call__(self, seq, initial_state=None, training=None):
        seq = np.asarray(seq, dtype=np.float64)
        n, T, _ = seq.shape
        U = self.recurrent_kernel.shape[0]
        h = np.broadcast_to(np.asarray(initial_state[0], dtype=np.float64), (n, U)).copy()
        c = np.broadcast_to(np.asarray(initial_state[1], dtype=np.float64), (n, U)).copy()
        out = np.zeros((n, T, U))
        for t in range(T):
            z = seq[:, t] @ self.kernel + h @ self.recurrent_kernel + self.bias
            i, f, g, o = _sigmoid(z[:, :U]), _sigmoid(z[:, U:2 * U]), np.tanh(z[:, 2 * U:3 * U]), _sigmoid(z[:, 3 * U:])
            c = f * c + i * g
            h = o * np.tanh(c)
            out[:, t] = h
        return out, h, c


def cases():
    rng = np.random.Generator(np.random.PCG64(835))
    out = {}
    # graph 2 is empty, graph 3 has one node
    sizes = [4, 3, 0, 1, 6]
    ids = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    for name, F, node_ids, iters in [("shuffled_f5_it3", 5, ids[rng.permutation(ids.size)], 3),
                                     ("sorted_f1_it1", 1, ids, 1),
                                     ("shuffled_f1_it4", 1, ids[rng.permutation(ids.size)], 4),
                                     ("one_graph_f5_it3", 5, np.zeros(6, dtype=np.int32), 3),
                                     ("sorted_f5_it1", 5, ids, 1)]:
        out[name] = dict(x=rng.normal(size=(node_ids.size, F)) * 1.5, node_graph_index=node_ids,
                         kernel=rng.normal(size=(2 * F, 4 * F)) * 0.6, recurrent_kernel=rng.normal(size=(F, 4 * F)) * 0.6,
                         bias=rng.normal(size=4 * F) * 0.3, num_iterations=iters)
    return out


def run_reference():
    tfg, tf, tfs, backend = load_reference()
    from tf_geometric.nn.pool.set2set import set2set
    blob = {"__backend__": np.array(backend), "__cases__": np.array(sorted(cases()))}
    for name, c in cases().items():
        lstm = NumpyLSTM(c["kernel"], c["recurrent_kernel"], c["bias"])
        x = tf.constant(c["x"]) if hasattr(tf, "constant") else c["x"]
        y = set2set(x, c["node_graph_index"], lstm, int(c["num_iterations"]))
        for k, v in c.items():
            blob["{}::{}".format(name, k)] = np.asarray(v)
        blob["{}::output".format(name)] = np.asarray(y, dtype=np.float64)
    return blob


if __name__ == "__main__":
    blob = run_reference()
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
