# coding=utf-8
"""2-layer LSTMGraphSage with per-layer neighbour sampling (k = 25, 10) on a PPI-shaped synthetic graph: the sampled demo of
examples/demo_graph_sage.py with the LSTM aggregator (reference layers.LSTMGraphSage).  Every forward draws a new edge
list whose CSR plan the sampler attaches, so the step is sampler -> plan -> x @ kernel -> fused gather/recurrence kernel ->
backward through time, with no sort.

    python examples/demo_graph_sage_lstm.py [--steps 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd.utils import RandomNeighborSampler   # noqa: E402
from demo_graph_sage import ppi_shaped, micro_f1   # noqa: E402

NUM_SAMPLED = [25, 10]


def main(steps=5, quiet=False, units=64, nodes=2200):
    torch.manual_seed(0)
    g = ppi_shaped(1, seed=1, n=nodes)[0]
    x, y = tfg._lib.as_f32(g["x"]), tfg._lib.as_f32(g["y"])
    sampler = RandomNeighborSampler(tfg._lib.as_i32(g["edge_index"]))
    sages = [tfg.layers.LSTMGraphSage(units, activation=tfg.relu, concat=True, seed=1).trainable(True),
             tfg.layers.LSTMGraphSage(units, activation=tfg.relu, concat=True, seed=2).trainable(True)]
    head = torch.nn.Linear(units, y.shape[1]).to(x.device)

    def forward():
        h = x
        for k, sage in zip(NUM_SAMPLED, sages):
            ei, _ = sampler.sample(k=k)
            h = sage([h, ei])
        return head(h)

    forward()       # builds the weights
    params = [p for s in sages for p in s.parameters()] + list(head.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)
    losses = []
    for step in range(steps):
        opt.zero_grad()
        logits = forward()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if not quiet:
            print("step {}  loss {:.4f}  micro-F1 {:.3f}".format(step, losses[-1], micro_f1(y.cpu().numpy(), logits.detach().cpu().numpy())))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    main(steps=ap.parse_args().steps)
