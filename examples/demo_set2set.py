# coding=utf-8
"""Graph classification with a Set2Set readout — the GCN stack of examples/demo_sag_pool_h.py (3 x GCN(128, relu)) read out
by tfg.layers.Set2Set instead of mean || max, then Dense(128, relu) -> Dense(num_classes), on the same seeded NCI1-shaped
stand-in (graphs of 10-50 nodes, a planted 6-cycle decides the class).

    python examples/demo_set2set.py [--steps 30] [--graphs 1000] [--per-graph]

Per step the readout costs num_iterations x (one sequence-LSTM launch + one attention launch); --per-graph runs the form in
which a graph does not depend on its batch (Set2Set(batch_graphs=True)).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd import autograd as AG   # noqa: E402
from demo_sag_pool_h import make_dataset, make_batch, _glorot   # noqa: E402

UNITS = 128


class Set2SetModel(object):
    def __init__(self, num_features, num_classes, num_iterations=4, batch_graphs=False, seed=0):
        dev = torch.device("cuda")
        self.gcns = [tfg.layers.GCN(UNITS, activation=tfg.relu, seed=seed + level) for level in range(3)]
        for level, gcn in enumerate(self.gcns):
            gcn._maybe_build([torch.empty(1, num_features if level == 0 else UNITS)])
        self.readout = tfg.layers.Set2Set(num_iterations=num_iterations, batch_graphs=batch_graphs, seed=seed + 10)
        self.readout._maybe_build([torch.empty(1, UNITS)])
        for layer in self.gcns + [self.readout]:
            layer.trainable(True)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        self.mlp = [(_glorot(gen, 2 * UNITS, 128, dev), torch.zeros(128, device=dev, requires_grad=True)),
                    (_glorot(gen, 128, num_classes, dev), torch.zeros(num_classes, device=dev, requires_grad=True))]

    def parameters(self):
        ps = []
        for layer in self.gcns + [self.readout]:
            ps += layer.parameters()
        for k, b in self.mlp:
            ps += [k, b]
        return ps

    def __call__(self, inputs, training=False):
        x, edge_index, node_graph_index, num_graphs = inputs
        h = x
        for gcn in self.gcns:
            h = gcn([h, edge_index, None], training=training)
        h = self.readout([h, node_graph_index, num_graphs], training=training)
        (k0, b0), (k1, b1) = self.mlp
        return AG.linear(AG.linear(h, k0, b0, tfg._lib.ACT_RELU), k1, b1)


def main(steps=30, graphs=1000, batch_size=256, lr=1e-3, per_graph=False, quiet=False, seed=0):
    torch.manual_seed(seed)
    data = make_dataset(graphs, seed)
    model = Set2SetModel(data.num_features, data.num_classes, batch_graphs=per_graph, seed=seed)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    batch = make_batch(data, list(rng.permutation(graphs)[:batch_size]))
    losses = []
    for step in range(steps):
        x, ei, gid, y, num_graphs = batch
        logits = model([x, ei, gid, num_graphs], training=True)
        loss = torch.nn.functional.cross_entropy(logits, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
        if not quiet:
            acc = float((logits.argmax(-1) == y).float().mean())
            print("step {:3d}  loss {:.4f}  batch accuracy {:.3f}".format(step, losses[-1], acc), flush=True)
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--graphs", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--per-graph", action="store_true")
    a = ap.parse_args()
    main(steps=a.steps, graphs=a.graphs, batch_size=a.batch_size, per_graph=a.per_graph)
