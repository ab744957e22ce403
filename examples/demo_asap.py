# coding=utf-8
"""Hierarchical ASAP graph classification — the MI355X counterpart of the reference's demo/demo_asap.py.

Same model: 3 x (GCN(64, relu) -> ASAP(ratio 0.5, drop_rate 0.1)), a mean || max readout after every level, the three
readouts summed, then Dense(64, relu) -> Dropout(0.5) -> Dense(num_classes).  The data is the seeded NCI1-shaped stand-in of
examples/demo_sag_pool_h.py (NCI1 itself needs a download).

    python examples/demo_asap.py [--epochs 20] [--graphs 4000] [--static] [--capture]

Every level's attention is one fused launch, every coarsened adjacency a sparse S^T A S; each pooled edge list carries its CSR
plan, so the GCN of the next level does not sort.

--static trains on fixed-shape batches instead: a GraphStore holds the graphs on the device, a StaticLoader hands on graph ids
from a device cursor, collate_static assembles them at capacities the host computed once, and every level is ASAP.pool_static (a
static batch in, a static batch out whose capacities shrink level by level: include/tfgx_asap_static.h) with the readouts the
batches carry and a loss masked by graph_mask — no host read anywhere in the step.  --capture (implies --static) records
ids -> batch -> three levels -> loss -> backward -> Adam once with tfg.CapturedTrainStep and replays it; the attention dropout
reads a device seed, so every replay draws new masks.  Without either flag the program is what it was.
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
from tf_geometric_amd import autograd as AG   # noqa: E402
from demo_sag_pool_h import make_dataset, make_batch, evaluate, _glorot, graph_store, make_static_step   # noqa: E402,F401

UNITS = 64


class ASAPModel(object):
    def __init__(self, num_features, num_classes, seed=0, drop_rate=0.1):
        dev = torch.device("cuda")
        self.gcns, self.asaps = [], []
        for level in range(3):
            self.gcns.append(tfg.layers.GCN(UNITS, activation=tfg.relu, seed=seed + 2 * level))
            self.asaps.append(tfg.layers.ASAP(ratio=0.5, drop_rate=drop_rate, seed=seed + 2 * level + 1))
            self.gcns[-1]._maybe_build([torch.empty(1, num_features if level == 0 else UNITS)])
            self.asaps[-1]._maybe_build([torch.empty(1, UNITS)])
        for layer in self.gcns + self.asaps:
            layer.trainable(True)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        self.mlp = [(_glorot(gen, 2 * UNITS, 64, dev), torch.zeros(64, device=dev, requires_grad=True)),
                    (_glorot(gen, 64, num_classes, dev), torch.zeros(num_classes, device=dev, requires_grad=True))]
        self.step = 0

    def parameters(self):
        ps = []
        for layer in self.gcns + self.asaps:
            ps += layer.parameters()
        for k, b in self.mlp:
            ps += [k, b]
        return ps

    def __call__(self, inputs, training=False):
        x, edge_index, node_graph_index, num_graphs = inputs
        edge_weight = None
        h = x
        out = None
        self.step += 1
        for level, (gcn, asap) in enumerate(zip(self.gcns, self.asaps)):
            h = gcn([h, edge_index, edge_weight], training=training)
            h, edge_index, edge_weight, node_graph_index = asap([h, edge_index, edge_weight, node_graph_index],
                                                                training=training, seed=3 * self.step + level)
            readout = torch.cat([tfg.nn.mean_pool(h, node_graph_index, num_graphs),
                                 tfg.nn.max_pool(h, node_graph_index, num_graphs)], dim=-1)
            out = readout if out is None else out + readout
        (k0, b0), (k1, b1) = self.mlp
        h = AG.linear(out, k0, b0, tfg._lib.ACT_RELU)
        if training:
            h = torch.nn.functional.dropout(h, 0.5, training=True)
        return AG.linear(h, k1, b1)

    def static(self, batch, training=False, levels=None):
        """The model on a StaticBatchGraph: one row of logits per SLOT (dead slots: the biases alone).  Level by level the pooled
        batch replaces its parent (and is appended to `levels` when a list is given)."""
        h, out = batch.x, None
        for gcn, asap in zip(self.gcns, self.asaps):
            h = gcn([h, batch.edge_index, batch.edge_weight], cache=batch.cache, training=training)
            batch = asap.pool_static(h, batch, training=training)
            h = batch.x
            if levels is not None:
                levels.append(batch)
            readout = torch.cat([batch.readout(h, "mean"), batch.readout(h, "max")], dim=-1)
            out = readout if out is None else out + readout
        (k0, b0), (k1, b1) = self.mlp
        h = AG.linear(out, k0, b0, tfg._lib.ACT_RELU)
        if training:
            h = torch.nn.functional.dropout(h, 0.5, training=True)
        return AG.linear(h, k1, b1)


def static_loss(model, batch, training=True):
    """Mean cross-entropy over the LIVE slots (a dead slot holds graph 0's label: torch.where on graph_mask)."""
    per_slot = torch.nn.functional.cross_entropy(model.static(batch, training=training), batch.y.reshape(-1), reduction="none")
    zero = torch.zeros((), dtype=per_slot.dtype, device=per_slot.device)
    return torch.where(batch.graph_mask, per_slot, zero).sum() / batch.counts[0].clamp(min=1).to(per_slot.dtype)


def train_static(model, data, train_idx, test_batches, args):
    """The --static / --capture route: the epochs of main() over fixed-shape batches."""
    store = graph_store(data, train_idx)
    loader = store.static_loader(args.batch_size, shuffle=True, seed=args.seed + 1)
    cap = store.static_capacities(args.batch_size)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, capturable=args.capture)
    step = make_static_step(model, store, loader, cap, opt, args.capture, loss=static_loss)
    print("batches: collate_static{}; capacities: {} rows and {} edges for {} slots".format(
        ", replayed" if args.capture else "", cap.n_cap, cap.e_cap, cap.batch_size), flush=True)
    for epoch in range(args.epochs):
        if epoch:
            loader.reshuffle(args.seed + 1 + epoch)           # in place: the replay reads the new order
        t0 = time.perf_counter()
        losses = torch.stack([step().detach().clone() for _ in range(loader.steps_per_epoch)])
        loss = float(losses.mean().item())                    # the one read of the epoch
        ms = (time.perf_counter() - t0) * 1e3 / loader.steps_per_epoch
        print("epoch {:3d}  loss {:.6f}  test accuracy {:.4f}  ({:.2f} ms / step)".format(
            epoch, loss, evaluate(model, test_batches), ms), flush=True)


def train_step(model, opt, batch):
    x, ei, gid, y, num_graphs = batch
    logits = model([x, ei, gid, num_graphs], training=True)
    loss = torch.nn.functional.cross_entropy(logits, y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.item())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--epochs", type=int, default=20)
    p.add_argument("--batch-size", type=int, default=512)
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--static", action="store_true", help="fixed-shape batches: collate_static and ASAP.pool_static")
    p.add_argument("--capture", action="store_true", help="replay the whole step from one hipGraph (implies --static)")
    args = p.parse_args()
    torch.manual_seed(args.seed)
    data = make_dataset(args.graphs, args.seed)
    n_test = len(data.graphs) // 10
    train_idx = np.arange(n_test, len(data.graphs))
    test_batches = [make_batch(data, list(range(i, min(i + args.batch_size, n_test)))) for i in range(0, n_test, args.batch_size)]
    model = ASAPModel(data.num_features, data.num_classes, seed=args.seed)
    if args.static or args.capture:
        return train_static(model, data, train_idx, test_batches, args)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.Generator(np.random.PCG64(args.seed + 1))
    for epoch in range(args.epochs):
        order = rng.permutation(train_idx)
        batches = [make_batch(data, list(order[i:i + args.batch_size])) for i in range(0, order.size, args.batch_size)]
        t0 = time.perf_counter()
        losses = [train_step(model, opt, b) for b in batches]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / len(batches)
        print("epoch {:3d}  loss {:.4f}  test accuracy {:.4f}  ({:.1f} ms / step)".format(
            epoch, float(np.mean(losses)), evaluate(model, test_batches), ms), flush=True)


if __name__ == "__main__":
    main()
