# coding=utf-8
"""2-layer GCN trained with DropEdge (https://openreview.net/forum?id=Hkx1qkrKPr) on a synthetic planted-partition graph.

Every training step draws a new edge list: `tfg.layers.DropEdge` drops edges on the device and hands the layers the
dropped list's CSR plan and transposed plan, derived from the full graph's without sorting.  The full
graph's plan is built once, before the loop; the log ends with the number of sorts the training steps ran (0).

    python examples/demo_drop_edge.py [--nodes 20000] [--steps 40] [--rate 0.5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd.plan import CsrPlan   # noqa: E402


def planted_partition(n, classes=6, degree=12, features=32, seed=0):
    """Nodes of a class are mostly linked to each other (80 %); features are noise plus a class direction."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, classes, n)
    order = np.argsort(y, kind="stable")
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    a = rng.integers(0, n, n * degree // 2)
    near = order[np.clip(pos[a] + rng.integers(-30, 31, a.shape[0]), 0, n - 1)]
    b = np.where(rng.random(a.shape[0]) < 0.8, near, rng.integers(0, n, a.shape[0]))
    a, b = a[a != b], b[a != b]
    edge_index = np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int32)
    centers = rng.standard_normal((classes, features)).astype(np.float32)
    x = (rng.standard_normal((n, features)) + centers[y]).astype(np.float32)
    return x, edge_index, y.astype(np.int64)


def main(nodes=20000, steps=40, rate=0.5):
    x_np, ei_np, y_np = planted_partition(nodes)
    classes = int(y_np.max()) + 1
    x = tfg._lib.as_f32(x_np)
    y = torch.as_tensor(y_np, device=x.device)
    edge_index = tfg._lib.as_i32(ei_np)
    edge_weight = torch.ones(edge_index.shape[1], device=x.device)
    # the full graph's plan and transposed plan: built (sorted) once; DropEdge derives every step's plans from them
    plan = CsrPlan.build(edge_index, nodes, nodes)
    plan.transposed()
    tfg.plan.attach_plan(edge_index, plan)

    drop = tfg.layers.DropEdge(rate)
    gcn0, gcn1 = tfg.layers.GCN(32, activation=tfg.relu), tfg.layers.GCN(classes)

    def model(training):
        ei, w = drop([edge_index, edge_weight], training=training)
        cache = {}                                  # one dict per drawn graph: both layers share its normalised adjacency
        h = gcn0([x, ei, w], cache=cache, training=training)
        return gcn1([h, ei, w], cache=cache, training=training)

    model(False)                                    # builds the weights
    gcn0.trainable(True)
    gcn1.trainable(True)
    optimizer = torch.optim.Adam(gcn0.parameters() + gcn1.parameters(), lr=3e-2)
    train = torch.arange(0, nodes, 2, device=x.device)
    test = torch.arange(1, nodes, 2, device=x.device)

    sorts = []
    real_build = CsrPlan.build
    CsrPlan.build = staticmethod(lambda *a, **k: sorts.append(1) or real_build(*a, **k))
    try:
        for step in range(1, steps + 1):
            optimizer.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(True)[train], y[train])
            loss.backward()
            optimizer.step()
            print("step {} loss {:.4f}".format(step, float(loss.detach())))
    finally:
        CsrPlan.build = staticmethod(real_build)
    with torch.no_grad():
        acc = float((model(False)[test].argmax(-1) == y[test]).float().mean())
    print("test accuracy {:.4f}".format(acc))
    print("sorts during training: {}".format(len(sorts)))
    return acc


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rate", type=float, default=0.5)
    args = ap.parse_args()
    main(args.nodes, args.steps, args.rate)
