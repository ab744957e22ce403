# coding=utf-8
"""Graph classification fed by tfg.data.GraphStore: the model and the synthetic dataset of examples/demo_sag_pool_h.py, with
the minibatches assembled on the device.

The dataset is packed once (tfg.Graph -> GraphStore); every step's batch — features, edge list, node_graph_index, labels and
the CSR plans of the first GCN's forward and backward pass — then comes out of one kernel launch, with no sort and no host
synchronisation.  --host-batches builds the batches the way the other demos do (a Python loop over the graphs, numpy
concatenation, five host-to-device copies, plans sorted by the first layer), for comparison.

    python examples/demo_graph_store.py [--epochs 30] [--graphs 4000] [--host-batches]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tf_geometric_amd as tfg   # noqa: E402
from demo_sag_pool_h import NUM_LABELS, SAGPoolHModel, evaluate, make_batch, make_dataset, train_step   # noqa: E402


def to_graphs(data, indices):
    graphs = []
    for i in indices:
        node_labels, ei = data.graphs[i]
        x = np.zeros((node_labels.size, NUM_LABELS), dtype=np.float32)
        x[np.arange(node_labels.size), node_labels] = 1.0
        graphs.append(tfg.Graph(x, ei, y=data.labels[i:i + 1]))
    return graphs


def as_inputs(batch):
    """BatchGraph -> the (x, edge_index, node_graph_index, y, num_graphs) the demo's train_step / evaluate take."""
    return batch.x, batch.edge_index, batch.node_graph_index, batch.y, batch.num_graphs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--batch-size", type=int, default=512)
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--host-batches", action="store_true", help="build batches on the host (make_batch of demo_sag_pool_h)")
    args = p.parse_args()
    torch.manual_seed(args.seed)
    data = make_dataset(args.graphs, args.seed)
    n_test = len(data.graphs) // 10
    train_idx = np.arange(n_test, len(data.graphs))
    if args.host_batches:
        rng = np.random.Generator(np.random.PCG64(args.seed + 1))

        def train_batches(epoch):
            order = rng.permutation(train_idx)
            return (make_batch(data, list(order[i:i + args.batch_size])) for i in range(0, order.size, args.batch_size))

        def test_batches():
            return (make_batch(data, list(range(i, min(i + args.batch_size, n_test)))) for i in range(0, n_test, args.batch_size))
    else:
        train_store = tfg.data.GraphStore(to_graphs(data, train_idx))
        test_store = tfg.data.GraphStore(to_graphs(data, range(n_test)))

        def train_batches(epoch):
            return (as_inputs(b) for b in train_store.batches(args.batch_size, shuffle=True, seed=args.seed + 1 + epoch))

        def test_batches():
            return (as_inputs(b) for b in test_store.batches(args.batch_size))
    model = SAGPoolHModel(data.num_features, data.num_classes, seed=args.seed)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    print("batches: {}".format("host (make_batch)" if args.host_batches else "GraphStore.collate"), flush=True)
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = [train_step(model, opt, b) for b in train_batches(epoch)]       # batch assembly is inside the timed window
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / len(losses)
        print("epoch {:3d}  loss {:.4f}  test accuracy {:.4f}  ({:.1f} ms / step)".format(
            epoch, float(np.mean(losses)), evaluate(model, test_batches()), ms), flush=True)


if __name__ == "__main__":
    main()
